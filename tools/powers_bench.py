#!/usr/bin/env python3
"""Phase 1 of the key ceremony on the device, at a domain of 2^20 (and more with --log2 20,25, memory permitting):
  scale kernels   powers_scale_kernel in G1 and G2 over device arrays of m points (fk_g1/g2_scale_powers_dev + sync): points/s, products/s,
                  the fraction of fk_calibrate's rate of the multiplier running alone (same run), and the G1 per-point time over
                  g1_scale_kernel's (fk_g1_scale_dev, one 254-bit scalar for all points, same array, same run, alternating)
  contribute      fk_powers_contribute of the whole transcript (host arrays in, host arrays out)
  validate        fk_points_validate per array (host array in)
  update check    fk_powers_update_check, seed drawn by the library
  host            the references per point at a small size, scaled by count and labelled extrapolated
The transcript is made with the feature itself: contribute(new_powers(m), TAU, ALPHA, BETA), then one more contribution (X, Y, Z); the
update check of the second against the first must accept and the check of a transcript against an unrelated `before` must not (asserted).

Counted from the formulas of csrc/curve.hpp in products of Fq (an Fq2 product is 3, an Fq2 square 2): Xyzz::dbl 9 (G2 24), add_mixed_nz
10 (G2 28).  Every lane has its own 254-bit scalar, so a wave executes the addition in practically every step: 256 doublings and 256
additions per point, 4864 products in G1 and 13312 in G2.  Not counted: the lane's scalar (~130 products of Fr) and the inversion of
to_affine (~390 in G1), about a tenth more in G1.  g1_scale_kernel: a doubling per digit of the scalar's non-adjacent form but the top
one, an addition per further nonzero digit.
Every figure is a host clock around a call that blocks until its result is on the host, after a warm-up; min / median / max over
--repeats calls.  Lines are appended to --log as well; the last line is one JSON object."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('FK_MSM_PRECOMP', '0')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import api, ceremony, powers as PW  # noqa: E402

R = api.FR_MODULUS
DBL, MIX = (9, 24), (10, 28)                         # (G1, G2) products of Fq
PER_POINT = tuple(256 * (DBL[g] + MIX[g]) for g in (0, 1))
TAU, ALPHA, BETA = 0x1d5c2a7b3f90e4681a2c3e5f708192a3b4c5d6e7f8091a2b3c4d5e6f70819203 % R, 0x0a1b2c3d4e5f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e8f9 % R, 0x2f1e0d3c4b5a69788796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f1 % R
X, Y, Z = 0x2b0d3c5f7a91e46802c4d6f8a1b3c5d7e9f10325476980badcfe1032547698ba % R, 0x1a2b3c4d5e6f708192a3b4c5d6e7f8090a1b2c3d4e5f60718293a4b5c6d7e8f9 % R, 0x13579bdf02468ace13579bdf02468ace13579bdf02468ace13579bdf02468ace % R


def mont(v):
    return api.int_to_limbs(v * (1 << 256) % R)


def naf_products(k):
    """products of g1_scale_kernel per point for the scalar k: a doubling per digit but the top one, a mixed addition per further nonzero digit"""
    digits, nonzero = 0, 0
    while k:
        if k & 1:
            k -= 2 - (k & 3)
            nonzero += 1
        k >>= 1
        digits += 1
    return (digits - 1) * DBL[0] + (nonzero - 1) * MIX[0]


def timed(call, repeats):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter(); call()
        out.append(time.perf_counter() - t0)
    out.sort()
    return [out[0], out[len(out) // 2], out[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2', default='20')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-n', type=int, default=64)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'powers_bench.log'))
    args = ap.parse_args()
    log = open(args.log, 'a')

    def say(line):
        print(line, flush=True)
        log.write(line + '\n'); log.flush()

    ctx = fk.Context(0)
    rate = ctx.calibrate()['modmul_per_s']
    k_one = X                                           # the one scalar of g1_scale_kernel
    say('powers_bench: %s, %d calls per figure; products per point: powers_scale_kernel G1 %d G2 %d, g1_scale_kernel %d (expected G1 ratio %.2f); multiplier alone %.4g products/s'
        % (os.path.basename(fk.lib_path()), args.repeats, PER_POINT[0], PER_POINT[1], naf_products(k_one), PER_POINT[0] / naf_products(k_one), rate))
    res = dict(repeats=args.repeats, modmul_per_s=rate, products_per_point=dict(g1=PER_POINT[0], g2=PER_POINT[1], g1_scale_kernel=naf_products(k_one)), rows=[])

    def row(what, log_m, n, secs, per_point=None, **more):
        r = dict(what=what, log_m=log_m, n=n, ms=[s * 1e3 for s in secs], points_per_s=[n / s for s in reversed(secs)], **more)
        line = '%-16s 2^%-2d n %9d %11.3f ms (min %.3f max %.3f)  points/s min %.4g median %.4g max %.4g' % (what, log_m, n, secs[1] * 1e3, secs[0] * 1e3, secs[2] * 1e3,
                                                                                                               n / secs[2], n / secs[1], n / secs[0])
        if per_point:
            r.update(products_per_s=n * per_point / secs[1], of_multiplier_alone=n * per_point / secs[1] / rate)
            line += '  products_per_s %.4g  of_multiplier_alone %.3f' % (r['products_per_s'], r['of_multiplier_alone'])
        res['rows'].append(r)
        say(line + ''.join('  %s %s' % kv for kv in more.items()))
        return r

    # ---- the host references per point, at a small size
    small, _ = fk.contribute(ctx, fk.new_powers(args.host_n), mont(TAU), mont(ALPHA), mont(BETA))
    host = {}
    for name, pts in (('g1', small.tau_g1[:args.host_n]), ('g2', small.tau_g2)):
        t0 = time.perf_counter()
        ref = fk.scale_powers(None, pts, mont(X), mont(Y))
        host[name] = (time.perf_counter() - t0) / pts.shape[0]
        if ref.tobytes() != fk.scale_powers(ctx, pts, mont(X), mont(Y)).tobytes():
            raise SystemExit('device and host reference differ in ' + name)
        t0 = time.perf_counter()
        fk.validate_points(None, pts)
        host[name + '_validate'] = (time.perf_counter() - t0) / pts.shape[0]
    say('host             n %d: scale %.4f ms per G1 point, %.4f ms per G2 point; validate %.5f ms per G1 point, %.4f ms per G2 point (one core, generic double-and-add, the reference; device results equal)'
        % (args.host_n, host['g1'] * 1e3, host['g2'] * 1e3, host['g1_validate'] * 1e3, host['g2_validate'] * 1e3))
    res['host_ms_per_point'] = {k: v * 1e3 for k, v in host.items()}

    for lg in [int(v) for v in args.log2.split(',')]:
        m = 1 << lg
        t0 = time.perf_counter()
        first, _ = fk.contribute(ctx, fk.new_powers(m), mont(TAU), mont(ALPHA), mont(BETA))
        say('transcript       2^%-2d made by the feature from fixed secrets in %.3f s (includes the warm-up)' % (lg, time.perf_counter() - t0))
        # ---- the kernels alone, over device arrays
        per = {}
        for g2, name, pts in ((False, 'g1', first.tau_g1[:m]), (True, 'g2', first.tau_g2)):
            d_in, d_out = ctx.dev_alloc(pts.nbytes), ctx.dev_alloc(pts.nbytes)
            ctx.upload(d_in, pts)

            def run_powers():
                PW.scale_powers_dev(ctx, d_in, m, mont(X), mont(Y), 0, d_out, g2=g2)
                ctx.sync()

            def run_one():
                ceremony.scale_g1_dev(ctx, d_in, m, mont(k_one), d_out)
                ctx.sync()
            if g2:
                per[name] = timed(run_powers, args.repeats)
            else:                                                  # alternating with g1_scale_kernel over the same array
                run_powers(); run_one()
                a, b = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter(); run_powers(); a.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); run_one(); b.append(time.perf_counter() - t0)
                a.sort(); b.sort()
                per[name], per['one'] = [a[0], a[len(a) // 2], a[-1]], [b[0], b[len(b) // 2], b[-1]]
            row('scale kernel ' + name, lg, m, per[name], PER_POINT[1 if g2 else 0], host_extrapolated_s=host[name] * m)
            if not g2:
                row('g1_scale_kernel', lg, m, per['one'], naf_products(k_one))
                ratio = per['g1'][1] / per['one'][1]
                say('                 2^%-2d powers_scale_kernel<G1> / g1_scale_kernel per point: %.3f measured, %.3f by the product counts' % (lg, ratio, PER_POINT[0] / naf_products(k_one)))
                res['rows'].append(dict(what='g1 ratio', log_m=lg, measured=ratio, by_products=PER_POINT[0] / naf_products(k_one)))
            ctx.dev_free(d_in); ctx.dev_free(d_out)
        # ---- whole calls
        n_all = (2 * m - 1) + 3 * m
        out = {}

        def run_contribute():
            out['after'], out['pub'] = fk.contribute(ctx, first, mont(X), mont(Y), mont(Z))
        row('contribute', lg, n_all, timed(run_contribute, args.repeats), host_extrapolated_s=host['g1'] * (4 * m - 1) + host['g2'] * m)
        after, pub = out['after'], out['pub']
        for name in ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1'):
            pts = getattr(after, name)
            rep = []
            secs = timed(lambda: rep.append(fk.validate_points(ctx, pts)), args.repeats)
            if not rep[-1].ok:
                raise SystemExit('a point of the transcript the feature made is bad: %s %r' % (name, rep[-1]))
            row('validate ' + name, lg, pts.shape[0], secs, host_extrapolated_s=host['g2_validate' if name == 'tau_g2' else 'g1_validate'] * pts.shape[0])
        rep = []
        secs = timed(lambda: rep.append(fk.check_update(ctx, first, after, pub, m)), args.repeats)
        if not (rep[-1].accept and all(rep[-1].flags().values()) and all(rep[-1].after.flags().values())):
            raise SystemExit('the update check rejects an honest update: %r %r' % (rep[-1].flags(), rep[-1].after.flags()))
        wrong = fk.check_update(ctx, after, after, pub, m)            # `after` is not `after` with (X, Y, Z) applied
        if wrong.accept or wrong.step_tau or not wrong.after.accept:
            raise SystemExit('the update check accepts an update from the wrong transcript')
        row('update check', lg, n_all, secs, flags='asserted')
        del first, after, out
        ctx.trim()
    ctx.close()
    say(json.dumps(res))


if __name__ == '__main__':
    main()
