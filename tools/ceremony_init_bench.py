#!/usr/bin/env python3
"""The initial key from a powers-of-tau transcript on the device, at domains of 2^20 (and 2^25 with --log2 20,25):
  transforms   fk_g1_ntt_dev over three arrays' worth of points (one timed) and fk_g2_ntt_dev, inverse, in place, each alone
  derivation   fk_key_from_powers (FK_KEY_NO_LEVELS) of a synthetic circuit that fills the domain
  combination  the derivation less its four transforms: the sums per variable, h, the copies and the host's column build (by difference)
  check        fk_powers_check, seed drawn by the library
and beside them the expectation from counted Montgomery products at fk_calibrate's rate of the multiplier running alone, taken in the
same run, and the host reference (fk_key_from_powers_host) at 2^8, scaled by the operation count.

Counted from the formulas of csrc/curve.hpp, in products of Fq (an Fq2 product is 3, an Fq2 square 2): Xyzz::dbl 9 (G2 24), Xyzz::add 14
(G2 40), add_mixed_nz 10 (G2 28).  A butterfly multiplies by a 254-bit twiddle: 254 doublings and on average 127 additions, then its own
two additions.  A term of a combination with coefficient ONE or r - 1 is one mixed addition; any other coefficient is 254 doublings, 127
mixed additions and one addition.  The lanes of a wave take the addition of a step together whenever any of them has the bit, so a wave
can spend up to 254 additions where the count says 127: achieved / expected of about 1.4 is that, not a stall.

The transcript is generated points, not powers of one tau: the work does not depend on it, the check's flags do (they are not asserted).
The circuit: every gate has A = (c, v1) + (1, v2), B = (1, v3) with every fourth gate one more term (c', v4), C = (1, v5) and in every
eighth gate (1, ONE); the v are spread over the variables, c and c' full-width values, so ONE's column is long (folded in segments).
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
import numpy as np  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import api, ceremony_init as CI  # noqa: E402

DBL, ADD, MIX = (9, 24), (14, 40), (10, 28)          # (G1, G2) products of Fq
BITS = 254


def butterfly(g):
    return BITS * DBL[g] + BITS // 2 * ADD[g] + 2 * ADD[g]


def term(g, full):
    return BITS * DBL[g] + BITS // 2 * MIX[g] + ADD[g] if full else MIX[g]


def mont(v):
    return api.int_to_limbs(v * (1 << 256) % api.FR_MODULUS)


def circuit(log_m):
    """(R1cs, terms of A, B, C as (ONE-like, full-width) counts) for a domain of 2^log_m: gates + inputs = 2^log_m exactly"""
    nin = 2
    gates = (1 << log_m) - nin
    naux = gates
    nv = nin + naux
    g = np.arange(gates, dtype=np.uint64)
    c1, c2 = mont(0x2b0d3c5f7a91e46802c4d6f8a1b3c5d7e9f10325476980badcfe1032547698ba % api.FR_MODULUS), mont(api.FR_MODULUS - 7)
    one = mont(1)

    def var(mult, add):
        return ((g * np.uint64(mult) + np.uint64(add)) % np.uint64(nv - 1) + np.uint64(1)).astype(np.uint32)
    # A: two terms per gate
    a_ptr = np.arange(gates + 1, dtype=np.uint64) * 2
    a_col = np.stack([var(7, 3), var(13, 5)], 1).reshape(-1)
    a_val = np.tile(np.stack([c1, one]), (gates, 1))
    # B: one term, every fourth gate two
    extra = (g % 4 == 0)
    b_cnt = 1 + extra.astype(np.uint64)
    b_ptr = np.concatenate([[0], np.cumsum(b_cnt)]).astype(np.uint64)
    b_col = np.zeros(int(b_ptr[-1]), np.uint32)
    b_val = np.tile(one, (int(b_ptr[-1]), 1))
    b_col[b_ptr[:-1]] = var(11, 1)
    b_col[b_ptr[:-1][extra] + 1] = var(17, 9)[extra]
    b_val[b_ptr[:-1][extra] + 1] = c2
    # C: one term, every eighth gate ONE as well
    extra_c = (g % 8 == 0)
    c_cnt = 1 + extra_c.astype(np.uint64)
    c_ptr = np.concatenate([[0], np.cumsum(c_cnt)]).astype(np.uint64)
    c_col = np.zeros(int(c_ptr[-1]), np.uint32)
    c_col[c_ptr[:-1]] = (g % np.uint64(naux) + np.uint64(nin)).astype(np.uint32)
    c_val = np.tile(one, (int(c_ptr[-1]), 1))
    r1cs = fk.R1cs(nin, naux, (a_ptr, a_col, a_val), (b_ptr, b_col, b_val), (c_ptr, c_col, c_val))
    counts = dict(A=(gates + nin, gates), B=(gates, int(extra.sum())), C=(int(c_ptr[-1]), 0))       # A's ONE terms include the inputs' own rows
    return r1cs, counts


def combination_products(counts):
    """a_all (A over G1), b1_all (B over G1), b2_all (B over G2), e (A, B and C over G1)"""
    def s(name, g):
        ones, full = counts[name]
        return ones * term(g, False) + full * term(g, True)
    return 2 * s('A', 0) + 2 * s('B', 0) + s('B', 1) + s('C', 0)


def timed(call, repeats):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter(); call()
        out.append(time.perf_counter() - t0)
    out.sort()
    return [out[0], out[len(out) // 2], out[-1]]


def points(ctx, n, g2, seed):
    d = ctx.dev_alloc(n * (128 if g2 else 64))
    (ctx.gen_points_g2_dev if g2 else ctx.gen_points_g1_dev)(d, n, seed)
    out = ctx.download(d, n * (128 if g2 else 64)).reshape(n, -1)
    ctx.dev_free(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2', default='20')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--host-log2', type=int, default=8)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'ceremony_init_bench.log'))
    args = ap.parse_args()
    log = open(args.log, 'a')

    def say(line):
        print(line, flush=True)
        log.write(line + '\n'); log.flush()

    ctx = fk.Context(0)
    rate = ctx.calibrate()['modmul_per_s']
    say('ceremony_init_bench: %s, %d calls per figure; products per butterfly G1 %d G2 %d, per full-width term G1 %d G2 %d; multiplier alone %.4g products/s'
        % (os.path.basename(fk.lib_path()), args.repeats, butterfly(0), butterfly(1), term(0, True), term(1, True), rate))
    res = dict(repeats=args.repeats, modmul_per_s=rate, rows=[])

    def row(what, log_m, secs, products=None, **more):
        r = dict(what=what, log_m=log_m, ms=[s * 1e3 for s in secs], **more)
        line = '%-14s 2^%-2d %11.3f ms (min %.3f max %.3f)' % (what, log_m, secs[1] * 1e3, secs[0] * 1e3, secs[2] * 1e3)
        if products:
            r.update(products=products, expected_ms=products / rate * 1e3, achieved_over_expected=secs[1] / (products / rate))
            line += '  %.4g products: expected %.3f ms, achieved / expected %.2f' % (products, r['expected_ms'], r['achieved_over_expected'])
        res['rows'].append(r)
        say(line + ''.join('  %s %s' % kv for kv in more.items()))

    def transcript(m):
        return fk.PowersOfTau(points(ctx, 2 * m - 1, False, 1), points(ctx, m, True, 2), points(ctx, m, False, 3), points(ctx, m, False, 4), points(ctx, 1, True, 5))

    # the host reference at a small domain, and its products
    hl = args.host_log2
    r1cs, counts = circuit(hl)
    pw = transcript(1 << hl)
    t0 = time.perf_counter()
    host = fk.initial_key_host(pw, r1cs)
    host_s = time.perf_counter() - t0
    dev = fk.initial_key(ctx, pw, r1cs)
    for name in ('h', 'l', 'a', 'b_g1', 'b_g2'):
        if getattr(dev, name).tobytes() != getattr(host, name).tobytes():
            raise SystemExit('device and host reference differ in ' + name)
    dev.key.free()
    m = 1 << hl
    host_products = (m // 2) * hl * (3 * butterfly(0) + butterfly(1)) + combination_products(counts)
    say('host           2^%-2d %11.3f ms on %d threads for %.4g products (generic double-and-add, the reference; device arrays equal)' % (hl, host_s * 1e3, os.cpu_count(), host_products))
    res.update(host_log_m=hl, host_ms=host_s * 1e3, host_products=host_products)

    for lg in [int(v) for v in args.log2.split(',')]:
        m = 1 << lg
        r1cs, counts = circuit(lg)
        pw = transcript(m)
        stages = lg + 1                                        # the inverse's last stage multiplies both operands
        per = {}
        for g2, name in ((False, 'g1 transform'), (True, 'g2 transform')):
            d = ctx.dev_alloc(m * (128 if g2 else 64))
            (ctx.gen_points_g2_dev if g2 else ctx.gen_points_g1_dev)(d, m, 9)

            def run():
                (CI.g2_ntt_dev if g2 else CI.g1_ntt_dev)(ctx, d, lg, inverse=True)
                ctx.sync()
            per[g2] = timed(run, args.repeats)
            row(name, lg, per[g2], products=(m // 2) * stages * butterfly(1 if g2 else 0))
            ctx.dev_free(d)
            ctx.trim()
        secs = timed(lambda: CI.initial_key_dev(ctx, pw, r1cs)[0].free(), args.repeats)
        total = (m // 2) * stages * (3 * butterfly(0) + butterfly(1)) + combination_products(counts)
        row('derivation', lg, secs, products=total, host_scaled_s=host_s * total / host_products)
        rest = [max(s - 3 * per[False][1] - per[True][1], 0.0) for s in secs]
        row('combination', lg, rest, products=combination_products(counts), note='by_difference')
        row('check', lg, timed(lambda: fk.check_powers(ctx, pw, m), args.repeats))
        ctx.trim()
    ctx.close()
    say(json.dumps(res))


if __name__ == '__main__':
    main()
