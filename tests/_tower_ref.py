"""The reference of the tower tests (_tower_cases.py): Fq12 as Fq[w] / (w^12 - 18 w^6 + 82) on Python integers, with the schoolbook
products of oracle/bn254_ref.py (f12_mul, f12_inv, f12_pow).  There is no tower here, no Karatsuba and no sparse product: every
expected value is a polynomial-basis product of mapped operands.

The basis map is the only tower-aware code.  pairing.hpp builds Fq2 = Fq[u] / (u^2 + 1), Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + u,
Fq12 = Fq6[w] / (w^2 - v): an element is sum over k = 0..5 of (x_k + y_k u) w^k, the coefficient of w^k being c_h.c_j with k = 2 j + h
(c0.c0, c1.c0, c0.c1, c1.c1, c0.c2, c1.c2).  With u = w^6 - 9 its polynomial coefficients are c[k] = x_k - 9 y_k, c[k + 6] = y_k.

A tower element is a list of 12 integers in the order of the limb image: c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.
"""
import os
import re

import bn254_ref as ref

P = ref.Q
R_ORDER = ref.R
MONT_R = 1 << 256
RINV = pow(MONT_R, -1, P)
CONSTS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fawkes-crypto_amd', 'csrc', 'bn254_consts.h')

BN_X = (ref.ATE_LOOP_COUNT - 2) // 6          # the curve parameter: the optimal-ate count of the oracle is 6 x + 2
assert 36 * BN_X ** 4 + 36 * BN_X ** 3 + 24 * BN_X ** 2 + 6 * BN_X + 1 == P
assert 36 * BN_X ** 4 + 36 * BN_X ** 3 + 18 * BN_X ** 2 + 6 * BN_X + 1 == R_ORDER

ONE = ref.f12_one()
FINAL_EXPONENT = (P ** 12 - 1) // R_ORDER


def product_words(name):
    """the 32-bit words of a `#define NAME { 0x..u, ... }` of csrc/bn254_consts.h, little endian"""
    with open(CONSTS_H) as f:
        m = re.search(r'^#define\s+%s\s+\{([^}]*)\}' % re.escape(name), f.read(), re.M)
    assert m, name
    return [int(w.strip().rstrip('uU'), 16) for w in m.group(1).split(',')]


def words_value(words):
    return sum(w << (32 * i) for i, w in enumerate(words))


# ------------------------------------------------------------------------------------------------ the basis map
def w_index(t):
    """tower position t = 6 h + 2 j + i of the base coefficient c_h.c_j.c_i -> (k, i): component i of the Fq2 coefficient of w^k"""
    h, j, i = t // 6, (t % 6) // 2, t % 2
    return 2 * j + h, i


def to_poly(tw):
    c = [0] * 12
    for t in range(0, 12, 2):
        k, _ = w_index(t)
        x, y = tw[t], tw[t + 1]
        c[k] = (x - 9 * y) % P
        c[k + 6] = y % P
    return c


def from_poly(c):
    tw = [0] * 12
    for t in range(0, 12, 2):
        k, _ = w_index(t)
        tw[t], tw[t + 1] = (c[k] + 9 * c[k + 6]) % P, c[k + 6] % P
    return tw


def w_coeffs(co):
    """{k: (x, y)} -> the polynomial of sum (x + y u) w^k"""
    c = [0] * 12
    for k, (x, y) in co.items():
        c[k] = (x - 9 * y) % P
        c[k + 6] = y % P
    return c


def f6_embed(a):
    """an Fq6 element (6 integers, c0 c1 c2) as a tower element with c1 = 0"""
    return list(a) + [0] * 6


def f2_embed(a):
    return list(a) + [0] * 10


def mont_decode(images):
    return [m * RINV % P for m in images]


def mont_encode(values):
    return [v * MONT_R % P for v in values]


# ------------------------------------------------------------------------------------------------ the ate loops
ATE_T = words_value(product_words('FK_ATE_LOOP_T'))
assert ATE_T == 6 * BN_X * BN_X and ATE_T.bit_length() == 127


def miller_loop_lines(Pt, Qt):
    """f_{T,Q}(P), T = 6 x^2, with affine steps on the twist (ref.F2) and the line documented at the top of pairing.hpp,
    yP - lambda xP w + (lambda xR - yR) w^3, as a polynomial.  Pt, Qt: affine points or None."""
    if Pt is None or Qt is None:
        return list(ONE)
    F2 = ref.F2
    xp, yp = Pt
    xq, yq = Qt

    def line(lam, x0, y0):
        return w_coeffs({0: (yp, 0), 1: F2.neg(F2.muli(lam, xp)), 3: F2.sub(F2.mul(lam, x0), y0)})

    xr, yr, f = xq, yq, list(ONE)
    for bit in bin(ATE_T)[3:]:
        lam = F2.mul(F2.muli(F2.sqr(xr), 3), F2.inv(F2.muli(yr, 2)))
        f = ref.f12_mul(ref.f12_mul(f, f), line(lam, xr, yr))
        x3 = F2.sub(F2.sqr(lam), F2.muli(xr, 2))
        xr, yr = x3, F2.sub(F2.mul(lam, F2.sub(xr, x3)), yr)
        if bit == '1':
            lam = F2.mul(F2.sub(yr, yq), F2.inv(F2.sub(xr, xq)))
            f = ref.f12_mul(f, line(lam, xr, yr))
            x4 = F2.sub(F2.sub(F2.sqr(lam), xr), xq)
            xr, yr = x4, F2.sub(F2.mul(lam, F2.sub(xr, x4)), yr)
    return f


def miller_loop_linefunc(Pt, Qt):
    """the same bits with the oracle's own line and addition on the untwisted curve over Fq12 (ref._linefunc, ref._aff_add12,
    unchanged).  Each of its lines is the one above times -1: it shares no sign convention with miller_loop_lines, and agrees with
    it only after the final exponentiation."""
    if Pt is None or Qt is None:
        return list(ONE)
    q12, p12 = ref._twist(Qt), ref._cast_g1(Pt)
    r12, f = q12, list(ONE)
    for bit in bin(ATE_T)[3:]:
        f = ref.f12_mul(ref.f12_mul(f, f), ref._linefunc(r12, r12, p12))
        r12 = ref._aff_add12(r12, r12)
        if bit == '1':
            f = ref.f12_mul(f, ref._linefunc(r12, q12, p12))
            r12 = ref._aff_add12(r12, q12)
    return f
