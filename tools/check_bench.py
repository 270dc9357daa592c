#!/usr/bin/env python3
"""The R1CS check: what it costs, alone and inside a proof.
  check       fk_r1cs_check_dev on a resident witness (range kernel, evaluation of a, b, c, gate kernel, report), beside the evaluation
              alone (fk_r1cs_eval_dev + sync) -- the difference is what the check adds to an evaluation the prover runs anyway
  prove       fk_prove_r1cs_checked_dev beside fk_prove_r1cs_dev on the same witness, ALTERNATING in one process
at the benchmark's shape (the rollup transaction x --copies, tiled: domain 2^25 at the default 1741) and, for `check`, at the
4096-signature tiled shape (BASELINE configs[2]).

Every figure is a host clock around a call that blocks until its result is on the host, after a warm-up.  `check` rows: --repeats windows
of >= --window seconds; `prove` rows: --pairs alternating pairs, every sample kept.  min / median / max are printed; their spread is what
a difference has to beat.  The proof bytes of the two entry points are compared before anything is timed.  Lines are appended to --log as
well; the last line is one JSON object.  The gate kernel's own time is not a host clock's to give: take it from
`rocprofv3 --kernel-trace --stats -- python3 tools/check_bench.py --only check` (check_gates_kernel; 96 bytes x gates over its time is
its share of the HBM rate).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import bench  # noqa: E402  (data loading helpers only)
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import check as K  # noqa: E402


def windows(call, window, repeats):
    """seconds per call: sorted samples over `repeats` windows of >= `window` seconds each (the calls block)"""
    call()
    t0 = time.perf_counter(); call()
    one = max(time.perf_counter() - t0, 1e-6)
    k = max(1, int(math.ceil(window / one)))
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        out.append((time.perf_counter() - t0) / k)
    return sorted(out), k


def stats(samples):
    s = sorted(samples)
    return dict(min_ms=s[0] * 1e3, median_ms=s[len(s) // 2] * 1e3, max_ms=s[-1] * 1e3, spread=(s[-1] - s[0]) / s[len(s) // 2], n=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--copies', type=int, default=1741, help='rollup transactions of the benchmark shape (1741: domain 2^25)')
    ap.add_argument('--signatures', type=int, default=4096, help='copies of the eddsa verifier of the second shape (0: skip it)')
    ap.add_argument('--only', default='check,prove')
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'check_bench.log'))
    args = ap.parse_args()
    only = args.only.split(',')
    log = open(args.log, 'a')

    def say(line):
        print(line, flush=True)
        log.write(line + '\n'); log.flush()

    lib = K._lib()
    ctx = fk.Context(0)
    res = dict(library=os.path.basename(fk.lib_path()), window_s=args.window, repeats=args.repeats, rows=[])
    say('check_bench: %s, window %.2f s x %d, %d alternating pairs' % (res['library'], args.window, args.repeats, args.pairs))

    def check_rows(name, inst, copies, z):
        """the check alone on `copies` of `inst` (tiled), witness z resident"""
        dr = ctx.load_r1cs(inst, copies=copies)
        info = dr.info()
        gates = copies * inst.num_gates
        m = 1 << max(info['rows'] - 1, 1).bit_length()
        d_z = ctx.dev_alloc(z.nbytes)
        outs = [ctx.dev_alloc(m * 32) for _ in range(3)]
        try:
            ctx.upload(d_z, z)
            st = K.CheckReportStruct()

            def check():
                ctx._ck(lib.fk_r1cs_check_dev(ctx.handle, dr.handle, d_z, inst.num_gates, None, None, C.byref(st)))

            def evaluate():
                ctx.r1cs_eval_dev(dr, d_z, *outs)
                ctx.sync()

            check()
            if st.n_bad or st.n_range or not st.one_ok or st.gates != gates:
                raise SystemExit('%s: the witness does not satisfy the system (%d bad gates)' % (name, st.n_bad))
            for what, call in (('check', check), ('evaluation', evaluate), ('check', check), ('evaluation', evaluate)):
                s, k = windows(call, args.window, args.repeats)
                row = dict(shape=name, what=what, gates=gates, variables=info['num_vars'], matrix_terms=int(sum(info['nnz'])), calls_per_window=k,
                           gate_stream_bytes=96 * gates, gate_stream_floor_ms_at_8TBs=96 * gates / 8e12 * 1e3, **stats(s))
                res['rows'].append(row)
                say('%-22s %-10s gates %9d  %9.3f ms (min %.3f max %.3f, spread %5.2f %%, %d calls/window)'
                    % (name, what, gates, row['median_ms'], row['min_ms'], row['max_ms'], 100 * row['spread'], k))
        finally:
            for p in [d_z] + outs:
                ctx.dev_free(p)
        return dr, info

    inst, zs = bench.load_rollup_instance()
    copies = args.copies
    name = 'rollup x%d (tiled)' % copies
    z = bench.tile_witness(zs, inst.num_input, copies)
    dr = None
    try:
        if 'check' in only:
            dr, _ = check_rows(name, inst, copies, z)
        if 'prove' in only:
            if dr is None:
                dr = ctx.load_r1cs(inst, copies=copies)
            tox = {k: bench.mont(v) for k, v in bench.TOXIC.items()}
            r, s = bench.mont(0xA11CE), bench.mont(0xB0B)
            t0 = time.perf_counter()
            key, _ = ctx.setup(inst, copies=copies, **tox)
            say('%-22s key generated in %.1f s' % (name, time.perf_counter() - t0))
            d_z = ctx.dev_alloc(z.nbytes)
            try:
                ctx.upload(d_z, z)
                plain = lambda: ctx.prove_witness_dev(key, dr, d_z, r, s)                                  # noqa: E731
                checked = lambda: K.prove_checked(ctx, key, dr, d_z, r, s, group_rows=inst.num_gates)      # noqa: E731
                want = plain().tobytes()
                proof, rep = checked()
                if proof.tobytes() != want or not rep.ok:
                    raise SystemExit('%s: the checked proof differs from the plain one, or the report is not ok: %r' % (name, rep))
                plain(); checked()
                samples = dict(plain=[], checked=[])
                for i in range(args.pairs):
                    for what, call in ((('plain', plain), ('checked', checked)) if i % 2 == 0 else (('checked', checked), ('plain', plain))):
                        t0 = time.perf_counter(); call()
                        samples[what].append(time.perf_counter() - t0)
                for what in ('plain', 'checked'):
                    row = dict(shape=name, what='prove ' + what, samples_ms=[x * 1e3 for x in samples[what]], **stats(samples[what]))
                    res['rows'].append(row)
                    say('%-22s prove %-8s %9.3f ms (min %.3f max %.3f, spread %5.2f %%, %d samples)'
                        % (name, what, row['median_ms'], row['min_ms'], row['max_ms'], 100 * row['spread'], row['n']))
                d = stats(samples['checked'])['median_ms'] - stats(samples['plain'])['median_ms']
                res['checked_minus_plain_median_ms'] = d
                say('%-22s checked - plain (medians): %+.3f ms' % (name, d))
            finally:
                ctx.dev_free(d_z)
                key.free()
    finally:
        if dr is not None:
            dr.free()

    if 'check' in only and args.signatures:
        from helpers import eddsa_batch_inputs, r1cs_product
        _, one, _, z, _, _ = eddsa_batch_inputs(args.signatures)
        dr, _ = check_rows('eddsa x%d (tiled)' % args.signatures, r1cs_product(one), args.signatures, z)
        dr.free()
    ctx.close()
    say(json.dumps(res))


if __name__ == '__main__':
    main()
