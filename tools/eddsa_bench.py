#!/usr/bin/env python3
"""Device JubJub / EdDSA-Poseidon throughput (csrc/eddsa.hip), Poseidon parameters (4, 8, 54), at n = 1741, 4096, 2^16 and 2^20:
  verify  fk_eddsa_verify_batch_dev over resident signatures (made by the library's own signer; every row must accept)
  sign    fk_eddsa_sign_batch, host arrays in and out: the copies, the kernel and the host's s = rho + h sk mod Fs
  mul     fk_jubjub_mul_batch with the generator, host arrays in and out
Every figure is a host clock around work that ends in a stream synchronise, after a warm-up, over a window of at least --window seconds,
repeated --repeats times (min / median / max are printed: the spread is what a same-box A/B has to beat).  Montgomery products per second
= items/s x the product count DESIGN 3.7 derives, and its ratio to fk_calibrate's out[1] -- the library's multiplier running alone in
registers -- taken in the same run.  The last line is one JSON object.

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

T, F, P = 4, 8, 54
POSEIDON = (F * T + P) * 3 + (F + P) * T * T                   # 1250
INVERSE = 253 + 126                                            # a^(r - 2)
ROOT = 224 + 98 + 2 + 351 + 27 * 3 + 1                         # a^((t - 1) / 2), x and b, 27 Tonelli-Shanks rounds, the check
DECOMPRESS = 3 + INVERSE + ROOT + 3 + 250 * 8 + 114 * 7        # ..., the affine operand, [Fs] P
PRODUCTS = dict(verify=2 * DECOMPRESS + POSEIDON + 1 + 2 + 251 * 22 + 2,
                sign=2 * 251 * 15 + 1 + INVERSE + 4 + POSEIDON + 1,
                mul=256 * 15 + INVERSE + 2)


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
    ap.add_argument('--only', default='verify,sign,mul')
    ap.add_argument('--sizes', default='1741,4096,65536,1048576')
    args = ap.parse_args()
    only = set(args.only.split(','))
    sizes = [int(s) for s in args.sizes.split(',')]
    ctx = fk.Context(0)
    pp = fk.PoseidonParams(T, F, P)
    res = dict(variant=os.environ.get('FK_LIB_VARIANT', ''), products=PRODUCTS, window_s=args.window, repeats=args.repeats)
    cal = ctx.calibrate()
    res['calibrated_modmul_per_s'] = cal['modmul_per_s']
    print('library %s   calibrated multiplier alone: %.4g products/s' % (os.path.basename(fk.lib_path()), cal['modmul_per_s']))

    def report(op, n, secs, k):
        rate = [n / s for s in reversed(secs)]            # min, median, max of the RATE
        prod = rate[1] * PRODUCTS[op]
        res['%s_%d' % (op, n)] = dict(items=n, calls_per_window=k, ms=[s * 1e3 for s in secs], items_per_s=rate, products_per_s=prod,
                                      ratio_to_multiplier=prod / cal['modmul_per_s'], spread=(rate[2] - rate[0]) / rate[1])
        print('%-7s n = %8d  %10.3f ms  %.4g items/s (min %.4g max %.4g, spread %.2f %%)  %.4g products/s = %.3f of the multiplier alone'
              % (op, n, secs[1] * 1e3, rate[1], rate[0], rate[2], 100 * (rate[2] - rate[0]) / rate[1], prod, prod / cal['modmul_per_s']))

    rng = np.random.default_rng(2026)
    for n in sizes:
        # canonical limbs below 2^250 < Fs (sk, rho) and Montgomery images below 2^252 < r (m)
        sk, rho, m = (rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) for _ in range(3))
        sk[:, 3] >>= np.uint64(5); rho[:, 3] >>= np.uint64(5); m[:, 3] >>= np.uint64(3)
        if 'sign' in only:
            secs, k = timed(ctx, lambda: ctx.eddsa_sign(pp, sk, m, rho), args.window, args.repeats)
            report('sign', n, secs, k)
        if 'verify' in only:
            s, r_x, a_x = ctx.eddsa_sign(pp, sk, m, rho)
            bufs = [ctx.dev_alloc(32 * n) for _ in range(4)] + [ctx.dev_alloc(n)]
            for d, arr in zip(bufs, (s, r_x, a_x, m)):
                ctx.upload(d, arr)
            secs, k = timed(ctx, lambda: ctx.eddsa_verify_dev(pp, bufs[0], bufs[1], bufs[2], bufs[3], n, bufs[4]), args.window, args.repeats)
            accepted = int(ctx.download(bufs[4], n, np.uint8).sum())
            if accepted != n:
                raise SystemExit('verify: %d of %d of the library\'s own signatures accepted' % (accepted, n))
            report('verify', n, secs, k)
            for d in bufs:
                ctx.dev_free(d)
        if 'mul' in only:
            secs, k = timed(ctx, lambda: ctx.jubjub_mul(None, sk), args.window, args.repeats)
            report('mul', n, secs, k)
    cal2 = ctx.calibrate()
    res['calibrated_modmul_per_s_after'] = cal2['modmul_per_s']
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
