#!/usr/bin/env python3
"""Many proofs of one small circuit: proofs per second of the three ways to get `count` of them from one key, in one run on one box.

  loop      a loop over Context.prove_witness_dev (fk_prove_r1cs_dev), the witnesses resident on the device
  pipeline  fk_prove_r1cs_submit / _wait with two proofs in flight, the witnesses in host memory
  batch     batch.prove_batch_dev (fk_prove_batch_dev), the witnesses resident on the device as rows

on BASELINE configs[0] (the depth-32 Poseidon Merkle proof: 7362 gates, domain 2^13) and on a random system that fills a domain of 2^16,
for count in --counts.  Four distinct witnesses are dealt round robin, every proof has its own (r, s).  Before anything is timed, every
proof of `batch` and of `pipeline` is compared with `loop`'s, byte by byte.

Timing: a host clock around the whole of `count` proofs (every method ends synchronised: the proofs are in host memory), one warm-up of
every method at every count, then --repeats rounds that ALTERNATE the three methods; min / median / max proofs per second are printed, and
(max - min) / median of each method is the spread a difference has to beat.  --loop-cap N times the two per-proof methods over the first
min(count, N) proofs only (their rate per proof does not depend on how many follow); 0 = no cap.  Alongside: the batch call's per-stage
device times (fk_batch_timings, the median round), the plan under --budget-gib (the calls are given the same budget), and a probe of the G1 accumulation alone -- fk_batch_msm_dev over 2^13 - 1
points and uniform scalars, its accumulation kernel timed by the library's statistics events -- as a share of the v_mad_u64_u32 issue
peak fk_calibrate measures (additions counted from the digits' distribution: a lower bound, the top window is left out).
The last line is one JSON object.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import batch as B  # noqa: E402
import bn254_ref as ref  # noqa: E402
import fawkes_circuit as fc  # noqa: E402
import fixtures as fx  # noqa: E402
from helpers import r1cs_product, TOXIC  # noqa: E402

R = ref.R
MUL_PIPE_OPS_PER_MODMUL = 136      # bench.py: 8 x 8 products + 8 x 8 reduction products + 8 x (lo * INV)
MODMUL_PER_G1_MIXED_ADD = 10       # XYZZ mixed addition: 8 M + 2 S
DISTINCT = 4


def config0():
    inst = []
    for k in range(DISTINCT):
        rnd = random.Random(13 + k)
        inst.append(fc.poseidon_merkle_circuit(rnd.randrange(R), [rnd.randrange(R) for _ in range(32)], [rnd.randrange(2) for _ in range(32)])[0])
    return r1cs_product(fx.r1cs_to_csr(inst[0].r1cs())), [fx.witness_mont(c.z_in, c.z_aux) for c in inst]


def random16(gates):
    cs, z_in, z_aux = ref.random_r1cs(16, gates, 3, gates)
    rnd = random.Random(16)
    zs = [fx.witness_mont(z_in, z_aux)]
    for _ in range(DISTINCT - 1):          # perturbed: the prover does the same work on a witness that does not satisfy the system
        a = list(z_aux)
        for j in rnd.sample(range(len(a)), len(a) // 3):
            a[j] = rnd.randrange(R)
        zs.append(fx.witness_mont(z_in, a))
    return r1cs_product(fx.r1cs_to_csr(cs)), zs


def rate3(seconds, n):
    s = sorted(seconds)
    return [n / s[-1], n / s[len(s) // 2], n / s[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='1,8,64,256,1024')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--loop-cap', type=int, default=0)
    ap.add_argument('--circuits', default='config0,random16')
    ap.add_argument('--random-gates', type=int, default=60000)
    ap.add_argument('--budget-gib', type=float, default=64.0, help='scratch budget of the batch calls (and of the plan that is printed)')
    ap.add_argument('--methods', default='loop,pipeline,batch', help='a library built from a commit without the batch prover runs loop,pipeline')
    args = ap.parse_args()
    counts = [int(x) for x in args.counts.split(',')]
    methods = args.methods.split(',')
    opts = dict(scratch_budget_bytes=int(args.budget_gib * 2 ** 30))
    with_batch = 'batch' in methods
    ctx = fk.Context(0)
    tox = {k: fx.mont_fr(v) for k, v in TOXIC.items()}
    cal = ctx.calibrate()
    res = dict(counts=counts, repeats=args.repeats, loop_cap=args.loop_cap, calibrate=cal, circuits={})
    print('library %s   methods %s   repeats %d (methods alternate)   loop cap %d   proofs/s: min / median / max' % (os.path.basename(fk.lib_path()), args.methods, args.repeats, args.loop_cap))

    for name in args.circuits.split(','):
        r1cs, distinct = config0() if name == 'config0' else random16(args.random_gates)
        dk, _ = ctx.setup(r1cs, **tox)
        dr = ctx.load_r1cs(r1cs)
        c = dk.counts()
        nv = c['num_input'] + c['num_aux']
        print('%s: domain 2^%d, %d variables, queries l %d a %d b %d' % (name, c['m'].bit_length() - 1, nv, c['n_l'], c['n_a'], c['n_b']))
        rows = res['circuits'][name] = dict(log_m=c['m'].bit_length() - 1, counts={})
        for count in counts:
            rnd = random.Random(count)
            zs = np.ascontiguousarray(np.stack([distinct[i % DISTINCT] for i in range(count)]))
            rs = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in range(count)])
            ss = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in range(count)])
            d_z = ctx.dev_alloc(zs.nbytes)
            ctx.upload(d_z, zs)
            n_loop = min(count, args.loop_cap) if args.loop_cap else count

            def loop():
                return [ctx.prove_witness_dev(dk, dr, d_z + i * nv * 32, rs[i], ss[i]) for i in range(n_loop)]

            def pipeline():
                out, prev = [], ctx.prove_witness_submit(dk, dr, zs[0], rs[0], ss[0])
                for i in range(1, n_loop):
                    t = ctx.prove_witness_submit(dk, dr, zs[i], rs[i], ss[i])
                    out.append(ctx.prove_witness_wait(prev))
                    prev = t
                out.append(ctx.prove_witness_wait(prev))
                return out

            def batch():
                return B.prove_batch_dev(ctx, dk, dr, d_z, B.Z_ROWS, count, rs, ss, opts=opts, want_timings=True)

            # warm-up of every method at this count, and the comparison
            want = loop()
            if with_batch:
                got_b, _ = batch()
                assert all(got_b[i].tobytes() == want[i].tobytes() for i in range(n_loop)), 'batch differs from the per-proof prover'
            assert [p.tobytes() for p in pipeline()] == [p.tobytes() for p in want], 'pipeline differs from the per-proof prover'
            fns = dict(loop=loop, pipeline=pipeline, batch=batch)
            secs = {meth: [] for meth in methods}
            stages = []
            for _ in range(args.repeats):
                for meth in methods:
                    fn = fns[meth]
                    t0 = time.perf_counter()
                    out = fn()
                    secs[meth].append(time.perf_counter() - t0)
                    if meth == 'batch':
                        stages.append(out[1])
            ctx.dev_free(d_z)
            row = rows['counts'][count] = {}
            for meth in secs:
                n = count if meth == 'batch' else n_loop
                r3 = rate3(secs[meth], n)
                row[meth] = dict(proofs=n, proofs_per_s=r3, spread=(r3[2] - r3[0]) / r3[1])
            if not with_batch:
                print('%-9s count %5d   ' % (name, count) + '   '.join('%s %9.1f / %9.1f / %9.1f' % (meth, *row[meth]['proofs_per_s']) for meth in methods))
                continue
            stages.sort(key=lambda t: t['total_ms'])
            row['batch']['stages_ms'] = stages[len(stages) // 2]
            row['plan'] = B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], count, opts)
            best = max(row['loop']['proofs_per_s'][1], row['pipeline']['proofs_per_s'][1])
            row['batch_over_best'] = row['batch']['proofs_per_s'][1] / best
            # "ahead" = the batch's slowest round beats the better per-proof method's fastest round
            row['ahead_beyond_spread'] = row['batch']['proofs_per_s'][0] > max(row['loop']['proofs_per_s'][2], row['pipeline']['proofs_per_s'][2])
            print('%-9s count %5d   loop %9.1f / %9.1f / %9.1f   pipeline %9.1f / %9.1f / %9.1f   batch %9.1f / %9.1f / %9.1f   batch / best %.2fx   ahead beyond the spread: %s'
                  % (name, count, *row['loop']['proofs_per_s'], *row['pipeline']['proofs_per_s'], *row['batch']['proofs_per_s'], row['batch_over_best'], row['ahead_beyond_spread']))
            st = row['batch']['stages_ms']
            print('          batch stages (ms, median round): ' + '  '.join('%s %.3f' % (k[:-3], st[k]) for k in st)
                  + '   groups %d x %d, c = %d / %d' % (row['plan']['n_groups'], row['plan']['group'], row['plan']['window_bits_g1'], row['plan']['window_bits_g2']))
        dr.free(); dk.free()

    if not with_batch:
        print(json.dumps(res))
        ctx.close()
        return
    # the G1 accumulation alone
    n, count = (1 << 13) - 1, 256
    c = B.plan(1 << 13, 1, 1, 1, count)['window_bits_g1']
    W = 254 // c + 1
    d_bases, d_z = ctx.dev_alloc(64 * n), ctx.dev_alloc(32 * n * count)
    ctx.gen_points_g1_dev(d_bases, n, 5)
    ctx.gen_scalars_dev(d_z, n * count, 6, 0)
    B.msm_dev(ctx, d_bases, n, 0, d_z, B.Z_ROWS, n, count)
    acc_ms = []
    for _ in range(args.repeats):
        ctx.stats_reset()
        B.msm_dev(ctx, d_bases, n, 0, d_z, B.Z_ROWS, n, count)
        acc_ms.append(ctx.stats()['acc_g1']['ms'])
    acc_ms.sort()
    adds = count * n * (W - 1) * (1 - 2.0 ** -c)
    mads = adds * MODMUL_PER_G1_MIXED_ADD * MUL_PIPE_OPS_PER_MODMUL
    share = mads / (acc_ms[len(acc_ms) // 2] * 1e-3) / cal['mad_lane_ops_per_s']
    res['accumulation_probe'] = dict(n=n, count=count, window_bits=c, windows=W, additions_at_least=adds, acc_ms=acc_ms, share_of_mad_issue_peak=share,
                                     mad_lane_ops_per_s=cal['mad_lane_ops_per_s'])
    print('G1 accumulation probe: %d x %d uniform scalars, c = %d: %.3f / %.3f / %.3f ms for >= %.3g mixed additions = %.1f %% of the v_mad_u64_u32 issue peak (%.2f T lane-ops/s)'
          % (count, n, c, *acc_ms, adds, 100 * share, cal['mad_lane_ops_per_s'] / 1e12))
    ctx.dev_free(d_bases); ctx.dev_free(d_z)
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
