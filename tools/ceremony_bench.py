#!/usr/bin/env python3
"""Key ceremony on the device: one contribution (fk_key_contribute, FK_KEY_NO_LEVELS) and one check
(fk_key_contribution_check, seed drawn by the library) on synthetic keys of 2^20 and 2^25 points per array, and beside them
  scale kernel   fk_g1_scale_dev alone, in place, in Montgomery products per second -- counted from the formulas of csrc/curve.hpp:
                 9 per Xyzz::dbl, 10 per add_mixed_nz, and for to_affine 256 squarings + popcount(q - 2) products of the Fermat
                 inversion + 5 -- next to fk_calibrate's rate of the multiplier running alone, taken in the same run
  host           fk_g1_scale without a context (the reference), time per point at 2^10 points on one core.

A synthetic key's two deltas are unrelated points, so `delta_pair` does not hold for it or its descendants; before anything is timed the
check must report every other flag for the key the contribution made.  Every figure is a host clock around a call that blocks until its
result is on the host (the scale kernel: until fk_sync returns), after a warm-up, over windows of at least --window seconds, repeated
--repeats times; min / median / max are printed.  FK_MSM_PRECOMP=0 for the whole run: the check multiplies over the arrays themselves
and a contribution is asked without levels, so the 11 extra copies of every array a loader would derive are only in the way.
Lines are appended to --log as well; the last line is one JSON object.
"""
import argparse
import json
import math
import os
import sys
import time

os.environ.setdefault('FK_MSM_PRECOMP', '0')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import api, ceremony  # noqa: E402

X = 0x2b0d3c5f7a91e46802c4d6f8a1b3c5d7e9f10325476980badcfe1032547698ba % api.FR_MODULUS


def mont(v):
    return api.int_to_limbs(v * (1 << 256) % api.FR_MODULUS)


def naf(k):
    """(digits, nonzero digits) of the non-adjacent form of k"""
    n = nz = 0
    while k:
        if k & 1:
            k -= 2 - (k & 3)
            nz += 1
        k >>= 1
        n += 1
    return n, nz


def products_per_point(k):
    n, nz = naf(k)
    return 9 * (n - 1) + 10 * (nz - 1) + 256 + bin(api.FQ_MODULUS - 2).count('1') + 5


def timed(call, window, repeats):
    """seconds per call: [min, median, max] over `repeats` windows of >= `window` seconds each (the calls block)"""
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
    out.sort()
    return [out[0], out[len(out) // 2], out[-1]], k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2', default='20,25')
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'ceremony_bench.log'))
    args = ap.parse_args()
    log = open(args.log, 'a')

    def say(line):
        print(line, flush=True)
        log.write(line + '\n'); log.flush()

    ctx = fk.Context(0)
    x, xinv = mont(X), pow(X, -1, api.FR_MODULUS)
    per_point = products_per_point(xinv)
    cal = ctx.calibrate()
    say('ceremony_bench: %s, window %.2f s x %d; 1/x has %d digits, %d nonzero: %d products per point; multiplier alone %.4g products/s'
        % (os.path.basename(fk.lib_path()), args.window, args.repeats, *naf(xinv), per_point, cal['modmul_per_s']))
    res = dict(window_s=args.window, repeats=args.repeats, products_per_point=per_point, modmul_per_s=cal['modmul_per_s'], rows=[])

    def row(what, n, secs, k, **more):
        r = dict(what=what, n=n, calls_per_window=k, ms=[s * 1e3 for s in secs], points_per_s=[n / secs[2], n / secs[1], n / secs[0]], **more)
        res['rows'].append(r)
        say('%-12s n %9d  %10.3f ms (min %.3f max %.3f, %d calls/window)  points/s min %.4g median %.4g max %.4g%s'
            % (what, n, secs[1] * 1e3, secs[0] * 1e3, secs[2] * 1e3, k, *r['points_per_s'], ''.join('  %s %.4g' % kv for kv in more.items())))

    # the host reference on one core
    pts = np.zeros((1 << 10, 64), np.uint8)
    d = ctx.dev_alloc(pts.nbytes)
    ctx.gen_points_g1_dev(d, pts.shape[0], 7)
    pts = ctx.download(d, pts.nbytes).reshape(-1, 64)
    ctx.dev_free(d)
    t0 = time.perf_counter()
    want = ceremony.scale_g1(None, pts, mont(xinv))
    host_s = time.perf_counter() - t0
    if ceremony.scale_g1(ctx, pts, mont(xinv)).tobytes() != want.tobytes():
        raise SystemExit('the scale kernel and the host reference differ')
    say('host         n %9d  %10.3f ms: %.4g ms per point on one core (generic double-and-add, the reference)' % (pts.shape[0], host_s * 1e3, host_s * 1e3 / pts.shape[0]))
    res['host_ms_per_point'] = host_s * 1e3 / pts.shape[0]

    for lg in [int(v) for v in args.log2.split(',')]:
        n = 1 << lg
        big = lg >= 24
        window, repeats = (0.0, 3) if big else (args.window, args.repeats)
        # the scale kernel alone
        d = ctx.dev_alloc(n * 64)
        ctx.gen_points_g1_dev(d, n, 11)

        def scale():
            ceremony.scale_g1_dev(ctx, d, n, mont(xinv), d)
            ctx.sync()
        secs, k = timed(scale, window, repeats)
        row('scale kernel', n, secs, k, products_per_s=n * per_point / secs[1], of_multiplier_alone=n * per_point / secs[1] / cal['modmul_per_s'])
        ctx.dev_free(d)
        # contribution and check of a whole key: h has n - 1 points, l, a, b_g1, b_g2 n each
        key = ctx.synthetic_key(n, 2, n, n, n, seed=3)
        new, _ = ceremony.contribute(ctx, key, x)
        rep = ceremony.check(ctx, key, new)
        if not (rep.shape_equal and rep.fixed_equal and rep.delta_nonzero and rep.ratio_h and rep.ratio_l):
            raise SystemExit('2^%d: the check does not pass the key the contribution made: %r' % (lg, rep.flags()))
        new.free()

        def contribute():
            ceremony.contribute(ctx, key, x)[0].free()
        secs, k = timed(contribute, window, repeats)
        row('contribute', 2 * n - 1, secs, k)
        new, _ = ceremony.contribute(ctx, key, x)
        secs, k = timed(lambda: ceremony.check(ctx, key, new), window, repeats)
        row('check', 4 * n - 2, secs, k)
        new.free(); key.free()
        ctx.trim()
    ctx.close()
    say(json.dumps(res))


if __name__ == '__main__':
    main()
