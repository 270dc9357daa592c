#!/usr/bin/env python3
"""Device witness generation (csrc/witness.hip): the time to generate the witness of
  rollup   1741 rollup-style transactions (depth 32: 19298 variables each)
  eddsa    4096 eddsa-poseidon verifiers
  merkle   2^16 Poseidon Merkle proofs of depth 32
from their given rows, resident on the device, into the tiled witness -- and, in the same run, the time to upload that same witness from
pinned host memory (the step this replaces; through one pinned buffer of at most --pinned-mib, piece by piece) and fk_calibrate's
multiplier-alone rate.  The programs are traced from oracle/fawkes_circuit.py (tests/witness_trace.py); every copy runs the traced
instance's given row: the interpreter has no data-dependent control flow, so its time does not depend on the values.  Copy 0 of every
result is compared with the circuit builder's witness before anything is timed.

Every figure is a host clock around work that ends in a stream synchronise, after a warm-up, over a window of at least --window seconds,
repeated --repeats times: min / median / max are printed, and the spread is what a layout change would have to beat on one box.
Montgomery products per copy are counted from the program: one per term whose coefficient is not ONE, one per MUL and DIV0, 379 per
inversion, one per evaluated run of BITs.  The last line is one JSON object.
"""
import argparse
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import witness as W  # noqa: E402
import fawkes_circuit as fc  # noqa: E402
import fixtures as fx  # noqa: E402
import witness_trace  # noqa: E402

INVERSE = 253 + 126


def circuits():
    rnd = random.Random(1741)
    R = fc.R
    return dict(
        rollup=(1741, lambda: fc.rollup_tx_circuit(rnd.randrange(fc.FS), 500, 400, [rnd.randrange(R) for _ in range(32)], [rnd.randrange(2) for _ in range(32)],
                                                   rnd.randrange(fc.FS))),
        eddsa=(4096, lambda: fc.eddsa_circuit(rnd.randrange(fc.FS), rnd.randrange(R), rnd.randrange(fc.FS))[0]),
        merkle=(1 << 16, lambda: fc.poseidon_merkle_circuit(rnd.randrange(R), [rnd.randrange(R) for _ in range(32)], [rnd.randrange(2) for _ in range(32)])[0]))


def products_per_copy(p):
    c = p.counts()
    coeff = sum(1 for l in p.lcs for col, k in l if col and k != 1)
    evaluated = {}
    for v, (op, a0, a1) in enumerate(zip(p.op, p.arg0, p.arg1)):       # a combination costs its products every time it is evaluated
        if op == W.BIT:
            if not (v and p.op[v - 1] == W.BIT and p.arg0[v - 1] == a0):
                evaluated[a0] = evaluated.get(a0, 0) + 1
        elif op != W.GIVEN:
            for l in {a0, a1} if op in (W.MUL, W.DIV0) else {a0}:
                evaluated[l] = evaluated.get(l, 0) + 1
    for l in p.input_lc:
        evaluated[l] = evaluated.get(l, 0) + 1
    per_lc = [sum(1 for col, k in l if col and k != 1) for l in p.lcs]
    coeff_run = sum(per_lc[l] * n for l, n in evaluated.items())
    return dict(coefficient=coeff_run, coefficient_terms_stored=coeff, mul_div=c['MUL'] + c['DIV0'], inversion=INVERSE * (c['DIV0'] + c['INV0']), bit_runs=c['BIT_runs'],
                total=coeff_run + c['MUL'] + c['DIV0'] + INVERSE * (c['DIV0'] + c['INV0']) + c['BIT_runs'])


def timed(ctx, call, window, repeats):
    """seconds per call: [min, median, max] over `repeats` windows of >= `window` seconds each"""
    call(); ctx.sync()                         # warm-up (code load, clocks)
    t0 = time.perf_counter(); call(); ctx.sync()
    one = max(time.perf_counter() - t0, 1e-6)
    k = max(1, int(math.ceil(window * 1.15 / one)))
    out = []
    for _ in range(repeats):
        while True:
            t0 = time.perf_counter()
            for _ in range(k):
                call()
            ctx.sync()
            dt = time.perf_counter() - t0
            if dt >= window:
                break
            k = int(math.ceil(k * window * 1.25 / dt))
        out.append(dt / k)
    out.sort()
    return [out[0], out[len(out) // 2], out[-1]], k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default='rollup,eddsa,merkle')
    ap.add_argument('--copies', type=int, default=0, help='override the batch size of every circuit (rehearsals)')
    ap.add_argument('--pinned-mib', type=int, default=1024)
    args = ap.parse_args()
    ctx = fk.Context(0)
    cal = ctx.calibrate()
    res = dict(window_s=args.window, repeats=args.repeats, calibrated_modmul_per_s=cal['modmul_per_s'])
    print('library %s   calibrated multiplier alone: %.4g products/s' % (os.path.basename(fk.lib_path()), cal['modmul_per_s']))
    for name, (copies, build) in circuits().items():
        if name not in args.only.split(','):
            continue
        copies = args.copies or copies
        with witness_trace.trace() as t:
            cs = build()
        prog, given = t.program(cs)
        dp = W.load(ctx, prog)
        prods = products_per_copy(prog)
        n = prog.witness_len(copies)
        rows = np.tile(fk.api._fr_rows(given), (copies, 1))
        d_given, d_z = ctx.dev_alloc(max(rows.nbytes, 32)), ctx.dev_alloc(32 * n)
        ctx.upload(d_given, rows)
        W.generate_dev(ctx, dp, d_given, copies, d_z)
        ctx.sync()
        aux0 = ctx.download(d_z + 32 * (1 + copies * (prog.num_input - 1)), 32 * prog.num_aux, np.uint64)
        if aux0.tobytes() != fx.witness_mont(cs.z_in, cs.z_aux)[prog.num_input:].tobytes():
            raise SystemExit('%s: copy 0 of the device witness differs from the circuit builder\'s' % name)
        secs, k = timed(ctx, lambda: W.generate_dev(ctx, dp, d_given, copies, d_z), args.window, args.repeats)
        # the upload this replaces: the same number of bytes from pinned memory, piece by piece through one pinned buffer
        piece = min(32 * n, args.pinned_mib << 20)
        pinned = ctx.host_alloc((piece // 8,), np.uint64)
        pinned[:] = 1
        offs = list(range(0, 32 * n, piece))

        def upload():
            for o in offs:
                ctx.upload(d_z + o, pinned[:(min(piece, 32 * n - o)) // 8])
        up, uk = timed(ctx, upload, args.window, args.repeats)
        ctx.host_free(pinned)
        rate = prods['total'] * copies / secs[1]
        res[name] = dict(copies=copies, info=dp.info(), products_per_copy=prods, witness_bytes=32 * n, calls_per_window=k, generate_ms=[s * 1e3 for s in secs],
                         spread=(secs[2] - secs[0]) / secs[1], products_per_s=rate, ratio_to_multiplier=rate / cal['modmul_per_s'],
                         upload_ms=[s * 1e3 for s in up], upload_gb_per_s=32 * n / up[1] / 1e9, upload_calls_per_window=uk)
        print('%-7s %6d copies  %9.3f M products each  generate %9.3f ms (min %.3f max %.3f, spread %.2f %%)  %.4g products/s = %.3f of the multiplier alone'
              % (name, copies, prods['total'] / 1e6, secs[1] * 1e3, secs[0] * 1e3, secs[2] * 1e3, 100 * (secs[2] - secs[0]) / secs[1], rate, rate / cal['modmul_per_s']))
        print('%-7s witness %8.1f MB  pinned upload %9.3f ms (min %.3f max %.3f) = %.1f GB/s  generate / upload = %.2f'
              % ('', 32 * n / 1e6, up[1] * 1e3, up[0] * 1e3, up[2] * 1e3, 32 * n / up[1] / 1e9, secs[1] / up[1]))
        ctx.dev_free(d_given); ctx.dev_free(d_z)
        dp.free()
    res['calibrated_modmul_per_s_after'] = ctx.calibrate()['modmul_per_s']
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
