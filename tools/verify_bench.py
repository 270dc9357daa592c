#!/usr/bin/env python3
"""Batch verification of Groth16 proofs of one key: proofs per second of
  aggregate   fk_verify_aggregate_dev  one aggregated equation per batch, weights drawn by the library (csrc/verify_agg.hip)
  per-proof   fk_verify_batch_dev      one equation per proof (csrc/verify.hip)
at n = 64, 1741, 4096, 2^14, 2^16 honest proofs, and -- when a library built with -DFK_VERIFY_AGG_AFFINE is present as
libfawkes_hip_exp.so (`make EXP=1 EXTRA=-DFK_VERIFY_AGG_AFFINE`) -- of the aggregate path on the affine Miller loop at n = 4096, measured
by a child process of this run, alternating with the shipped build on the same device.

The batch is 64 distinct proofs of one statement repeated: neither path has control flow that depends on a proof's values (the
double-and-add of the aggregate path branches on the WEIGHTS, which are drawn per call).  Before anything is timed both paths must accept
every proof of the batch.  Every figure is a host clock around a call that blocks until the verdicts are on the host -- upload of the
proofs, kernels and the host tail included -- after a warm-up, over a window of at least --window seconds, repeated --repeats times (the
per-proof kernel at the largest size: one window).  min / median / max are printed; their spread is what a difference has to beat.
Lines are appended to --log as well; the last line is one JSON object.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import api, verify_agg  # noqa: E402
import agg_cases  # noqa: E402
import c_oracle  # noqa: E402

AFFINE_N = 4096


def timed(call, window, repeats):
    """seconds per call: [min, median, max] over `repeats` windows of >= `window` seconds each (the calls block)"""
    call()                                      # warm-up (code load, scratch growth, clocks)
    t0 = time.perf_counter(); call()
    one = max(time.perf_counter() - t0, 1e-6)
    k = max(1, int(math.ceil(window / one)))
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        out.append((time.perf_counter() - t0) / k)
    out.sort()
    return [out[0], out[len(out) // 2], out[-1]], k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='64,1741,4096,16384,65536')
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default='aggregate,per-proof')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'verify_bench.log'))
    ap.add_argument('--child', action='store_true', help='(internal) a measurement of another build inside a run: no header, no child of its own')
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(',')]
    only = args.only.split(',')
    lib_name = os.path.basename(fk.lib_path())
    log = open(args.log, 'a')

    def say(line):
        print(line, flush=True)
        log.write(line + '\n'); log.flush()

    c_oracle.build(); c_oracle.lib()
    st = agg_cases.random_statement(c_oracle)
    distinct_inputs, distinct_proofs = st.batch(64)
    ctx = fk.Context(0)
    if not args.child:
        say('verify_bench: %s, window %.2f s x %d, %d public inputs, 64 distinct proofs repeated' % (lib_name, args.window, args.repeats, distinct_inputs.shape[1]))
    res = dict(library=lib_name, window_s=args.window, repeats=args.repeats, rows=[])

    def measure(n, what, repeats=None, window=None):
        reps = -(-n // 64)
        inputs, proofs = np.tile(distinct_inputs, (reps, 1, 1))[:n], np.tile(distinct_proofs, (reps, 1))[:n]
        if what == 'aggregate':
            accept, wf, rep = verify_agg.verify_aggregate(ctx, st.vkb, inputs, proofs)
            if not (accept and wf.all()):
                raise SystemExit('aggregate: an honest batch of %d was not accepted' % n)
            call = lambda: verify_agg.verify_aggregate(ctx, st.vkb, inputs, proofs)      # noqa: E731
        else:
            if not api.verify_batch(ctx, st.vkb, inputs, proofs).all():
                raise SystemExit('per-proof: an honest batch of %d was not accepted' % n)
            call = lambda: api.verify_batch(ctx, st.vkb, inputs, proofs)                 # noqa: E731
        secs, k = timed(call, window or args.window, repeats or args.repeats)
        row = dict(path=what, library=lib_name, n=n, calls_per_window=k, ms=[s * 1e3 for s in secs], proofs_per_s=[n / secs[2], n / secs[1], n / secs[0]],
                   spread=(secs[2] - secs[0]) / secs[1])
        res['rows'].append(row)
        say('%-10s %-22s n %6d  %10.3f ms (min %.3f max %.3f, spread %5.2f %%, %d calls/window)  proofs/s min %.4g median %.4g max %.4g'
            % (what, lib_name, n, secs[1] * 1e3, secs[0] * 1e3, secs[2] * 1e3, 100 * row['spread'], k, *row['proofs_per_s']))
        return row

    for n in sizes:
        if 'aggregate' in only:
            measure(n, 'aggregate')
        if 'per-proof' in only:
            big = n == max(sizes) and n >= 1 << 16
            measure(n, 'per-proof', repeats=1 if big else None, window=4 * args.window if big else None)

    exp = os.path.join(os.path.dirname(fk.lib_path()), 'libfawkes_hip_exp.so')
    if not args.child and 'aggregate' in only:
        if os.path.exists(exp) and not os.environ.get('FK_LIB_VARIANT'):
            say('A/B at n = %d, alternating: %s (affine Miller loop, -DFK_VERIFY_AGG_AFFINE) in a child process, then %s' % (AFFINE_N, os.path.basename(exp), lib_name))
            for _ in range(2):
                log.flush()
                child = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--sizes', str(AFFINE_N), '--only', 'aggregate', '--window', str(args.window),
                                        '--repeats', str(args.repeats), '--log', args.log], env=dict(os.environ, FK_LIB_VARIANT='exp'), stdout=subprocess.PIPE, text=True)
                if child.returncode:
                    raise SystemExit('the child that measures %s failed (exit %d)' % (os.path.basename(exp), child.returncode))
                print(child.stdout, end='', flush=True)
                res['rows'] += json.loads(child.stdout.strip().splitlines()[-1])['rows']
                measure(AFFINE_N, 'aggregate')
        else:
            say('no %s: the affine Miller loop build was not measured' % os.path.basename(exp))
    ctx.close()
    if args.child:
        print(json.dumps(res))
    else:
        say(json.dumps(res))


if __name__ == '__main__':
    main()
