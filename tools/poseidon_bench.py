#!/usr/bin/env python3
"""Device Poseidon throughput (csrc/poseidon.hip), t = 3 parameters (3, 8, 53):
  hash    2^22 two-input hashes, resident inputs and outputs
  tree    Merkle tree build at 2^20 and 2^24 leaves (every level kept)
  proofs  1741 x 32 proof-root steps (the rollup workload's witness: 1741 transactions, depth-32 proofs)
Every figure is a host clock around a stream synchronise, after a warm-up, over a window of at least --window seconds (default 0.5),
repeated --repeats times (min / median / max are printed: the spread is what a same-box A/B has to beat).  Montgomery products per
second = hashes/s x ((f t + p) 3 + (f + p) t^2) = hashes/s x 780, and its ratio to fk_calibrate's out[1] -- the library's multiplier
running alone in registers -- taken in the same run.  The last line is one JSON object.

A/B of a build variant (csrc/Makefile: EXP=1 EXTRA=-D...): run once plain and once with FK_LIB_VARIANT=exp, alternating, in one session.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fawkes_crypto_amd as fk  # noqa: E402

T, F, P = 3, 8, 53
PRODUCTS_PER_HASH = (F * T + P) * 3 + (F + P) * T * T


def timed(ctx, call, window, repeats):
    """seconds per call: [min, median, max] over `repeats` windows of >= `window` seconds each"""
    call(); ctx.sync()                         # warm-up (code load, clocks, scratch growth)
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
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--only', default='hash,tree20,tree24,proofs')
    ap.add_argument('--log2-hashes', type=int, default=22)
    args = ap.parse_args()
    only = set(args.only.split(','))
    ctx = fk.Context(0)
    pp = fk.PoseidonParams(T, F, P)
    res = dict(variant=os.environ.get('FK_LIB_VARIANT', ''), products_per_hash=PRODUCTS_PER_HASH,
               window_s=args.window, repeats=args.repeats)
    cal = ctx.calibrate()
    res['calibrated_modmul_per_s'] = cal['modmul_per_s']
    print('library %s   calibrated multiplier alone: %.4g products/s' % (os.path.basename(fk.lib_path()), cal['modmul_per_s']))

    def report(name, hashes, secs, k):
        rate = [hashes / s for s in reversed(secs)]            # min, median, max of the RATE
        prod = rate[1] * PRODUCTS_PER_HASH
        res[name] = dict(hashes=hashes, calls_per_window=k, ms=[s * 1e3 for s in secs], hashes_per_s=rate, products_per_s=prod,
                         ratio_to_multiplier=prod / cal['modmul_per_s'], spread=(rate[2] - rate[0]) / rate[1])
        print('%-8s %9d hashes  %9.3f ms  %.4g hashes/s (min %.4g max %.4g, spread %.2f %%)  %.4g products/s = %.3f of the multiplier alone'
              % (name, hashes, secs[1] * 1e3, rate[1], rate[0], rate[2], 100 * res[name]['spread'], prod, res[name]['ratio_to_multiplier']))

    if 'hash' in only:
        n = 1 << args.log2_hashes
        d_in, d_out = ctx.dev_alloc(64 * n), ctx.dev_alloc(32 * n)
        ctx.gen_scalars_dev(d_in, 2 * n, 7)
        secs, k = timed(ctx, lambda: ctx.poseidon_dev(pp, d_in, 2, n, d_out), args.window, args.repeats)
        report('hash', n, secs, k)
        ctx.dev_free(d_in); ctx.dev_free(d_out)
    for lg in (20, 24):
        if 'tree%d' % lg in only:
            n = 1 << lg
            d_nodes = ctx.dev_alloc(32 * (2 * n - 1))
            ctx.gen_scalars_dev(d_nodes, n, 11)
            secs, k = timed(ctx, lambda: ctx.merkle_tree_dev(pp, d_nodes, n, d_nodes), args.window, args.repeats)
            report('tree%d' % lg, n - 1, secs, k)
            ctx.dev_free(d_nodes)
    if 'proofs' in only:
        n, depth = 1741, 32
        d_l, d_s, d_i, d_o = ctx.dev_alloc(32 * n), ctx.dev_alloc(32 * n * depth), ctx.dev_alloc(8 * n), ctx.dev_alloc(32 * n)
        ctx.gen_scalars_dev(d_l, n, 13); ctx.gen_scalars_dev(d_s, n * depth, 17)
        ctx.upload(d_i, np.random.default_rng(19).integers(0, 1 << 32, n, dtype=np.uint64))
        secs, k = timed(ctx, lambda: ctx.merkle_proof_roots_dev(pp, d_l, d_s, d_i, depth, n, d_o), args.window, args.repeats)
        report('proofs', n * depth, secs, k)
        for d in (d_l, d_s, d_i, d_o):
            ctx.dev_free(d)
    cal2 = ctx.calibrate()
    res['calibrated_modmul_per_s_after'] = cal2['modmul_per_s']
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
