"""The XYZZ point formulas of csrc/curve.hpp on the device, against the affine group law of oracle/bn254_ref.py on Python integers.

Each formula is called directly by a thin kernel of the test-only library (csrc/fieldtest.hip), over every coordinate type the
product instantiates it with: Fq, FqL, FqC (G1) and Fq2, Fq2T<FqL>, Fq2C (G2).  The XYZZ result the device returns is brought to
affine form in Python (x = X / ZZ, y = Y / ZZZ, infinity if and only if ZZ is zero) and compared with the reference; every result
also satisfies ZZ^3 == ZZZ^2 and the range of its type ([0, p), lazy [0, 2p)).  to_affine and affine_neg_if are compared as field
values (canonical types bit for bit).  The two scalar multiplications, mul_scalar (the subgroup check of B in the verifiers: r B must
be infinity) and mul_affine_bits (w A and w C of the aggregate verifier), are compared with `G.mul` over the non-lazy types.

Accumulators are fed in non-trivial XYZZ form, (x l^2, y l^3, l^2, l^3) for a random l; in the lazy types every coordinate is
randomly lifted by p.  Exceptional cases, in every type: accumulator at infinity, addend at infinity (the all-zero buffer, and in a
lazy type its other images), P + P (the doubling branch), P + (-P), both of these with the accumulator's x and y in each of their
lazy representations (the `is_zero` branches must be taken when a difference is p, not 0), dbl of infinity, affine_neg_if on
infinity, on y = 0 and on y = p.

Known limit: the wrappers are separate kernels.  The formulas are the same text as in msm_accumulate_kernel and the bucket
reductions, the compiler's scheduling around them is not; the whole-MSM parity tests remain the check on that.
"""
import functools
import random

import pytest

import bn254_ref as ref
from _fieldtest import MONT_R, TYPES, FieldTestLib, check_element, first_limb_odd, hexel
from helpers import g1_bases, g2_bases

pytestmark = pytest.mark.gpu

LIB = FieldTestLib()        # the module-level guard: after one failed call nothing more is launched from this module

POINT_TYPES = [t for t in TYPES if t.points]
N_GENERAL = {False: 200, True: 100}      # G1, G2 cases per formula besides the exceptional ones
P = ref.Q


def curve(t):
    return (ref.G2, ref.F2) if t.fq2 else (ref.G1, ref.F1)


@functools.lru_cache(maxsize=None)
def base_points(fq2):
    if fq2:
        return tuple(ref.g2_from_raw_le(bytes(b)) for b in g2_bases(48))
    return tuple(ref.g1_from_raw_le(bytes(b)) for b in g1_bases(48))


class Enc:
    """canonical values -> the Montgomery limb images the device is given (lazy types: randomly lifted by p)"""

    def __init__(self, t, seed):
        self.t, self.rnd = t, random.Random(seed)
        self.G, self.F = curve(t)

    def base(self, v, lift=None):
        m = v * MONT_R % P
        if self.t.lazy and (self.rnd.randrange(2) if lift is None else lift):
            m += P
        return m

    def el(self, v, lift=None):
        return (self.base(v[0], lift), self.base(v[1], lift)) if self.t.fq2 else self.base(v, lift)

    def rand_el(self, nonzero=True):
        r = lambda: self.rnd.randrange(1 if nonzero else 0, P)
        return (r(), r()) if self.t.fq2 else r()

    def zero(self, lift=None):
        return self.el(self.F.zero, lift)

    def affine(self, pt, lift=None):
        if pt is None:
            return (self.zero(lift), self.zero(lift))
        return (self.el(pt[0], lift), self.el(pt[1], lift))

    def xyzz(self, pt, lift=None, junk=True):
        """(x l^2, y l^3, l^2, l^3); infinity: ZZ = ZZZ = 0, x and y anything"""
        F = self.F
        if pt is None:
            x, y = (self.rand_el(), self.rand_el()) if junk else (F.zero, F.zero)
            return (self.el(x), self.el(y), self.zero(lift), self.zero(lift))
        l = self.rand_el()
        l2 = F.sqr(l)
        l3 = F.mul(l2, l)
        return (self.el(F.mul(pt[0], l2), lift), self.el(F.mul(pt[1], l3), lift), self.el(l2), self.el(l3))


def pair_cases(t, seed, allow_b_inf=True):
    """(accumulator A, addend B, class) as affine points; the encodings are made by the caller"""
    G, _ = curve(t)
    pts, rnd = base_points(t.fq2), random.Random(seed)
    out = []
    for i in range(N_GENERAL[t.fq2]):
        out.append((pts[rnd.randrange(len(pts))], pts[rnd.randrange(len(pts))], 'general'))        # equal now and then: doubling
    for i in range(8):
        a = pts[i]
        out += [(None, a, 'accumulator at infinity'), (a, a, 'P + P'), (a, G.neg(a), 'P + (-P)'), (G.add(a, a), a, '2P + P')]
        if allow_b_inf:
            out += [(a, None, 'addend at infinity'), (None, None, 'both at infinity')]
    return out


def encode_pairs(t, op, seed):
    """cases of p_add_mixed / p_add_mixed_nz / p_add: (operands, A, B, class)"""
    e = Enc(t, seed)
    second = e.xyzz if op == 'p_add' else e.affine
    out = []
    for a, b, lab in pair_cases(t, seed, allow_b_inf=op != 'p_add_mixed_nz'):
        if lab == 'general':
            out.append((e.xyzz(a) + second(b), a, b, lab))
        if lab != 'general':
            lifts = (0, 1) if t.lazy else (0,)
            for la in lifts:            # the accumulator (and the addend) wholly in one representation: differences of exactly 0 or p
                for lb in lifts:
                    out.append((e.xyzz(a, la, junk=bool(la)) + second(b, lb), a, b, lab + (', lifted %d%d' % (la, lb) if t.lazy else '')))
    return out


def affine_of_result(t, g, F):
    """the device's XYZZ limb images -> (why it is malformed or None, affine point or None)"""
    lim = t.q
    vals = []
    for el in g:
        for v in (el if t.fq2 else (el,)):
            if v >= lim:
                return 'a coordinate is outside the range of its type', None
        vals.append(tuple(v * t.rinv % P for v in el) if t.fq2 else el * t.rinv % P)
    x, y, zz, zzz = vals
    if F.mul(F.sqr(zz), zz) != F.sqr(zzz):
        return 'ZZ^3 != ZZZ^2', None
    if F.is_zero(zz):
        return None, None
    return None, (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))


def run_points(t, op, mode, cases, expect):
    """cases: (operands, A, B, class); expect(which operation ran, A, B) -> the affine point"""
    G, F = curve(t)
    alt = LIB.alt(op) if mode == 'divergent' else op
    ops = [c[0] for c in cases]
    if len(ops) % 64 == 0:
        ops, cases = ops + ops[-1:], cases + cases[-1:]
    got = LIB.run(t, op, mode, ops)
    bad, arms = [], {op: 0, alt: 0}
    for (c, a, b, lab), g in zip(cases, got):
        which = op if mode != 'divergent' or first_limb_odd(t, c[0]) else alt
        arms[which] += 1
        want = expect(which, a, b)
        why, pt = affine_of_result(t, g, F)
        if why is None and pt != want:
            why = 'wrong point'
        if why:
            bad.append('%s [%s] %s: operands %s -> %s' % (which, lab, why, ' '.join(hexel(t, x) for x in c), ' '.join(hexel(t, x) for x in g)))
    print('%s %s %s: %d cases (%s)' % (t, op, mode, len(cases), ', '.join('%s %d' % kv for kv in arms.items())))
    if mode == 'divergent':
        assert min(arms.values()) > len(cases) // 8, 'divergent mode needs lanes in both arms: %r' % arms
    assert not bad, '%d of %d results wrong\n%s' % (len(bad), len(cases), '\n'.join(bad[:6]))


def group_expect(t):
    G, _ = curve(t)
    return lambda which, a, b: G.add(a, a) if which in ('p_dbl', 'p_dbl_affine') else G.add(a, b)


def test_library_offers_the_point_kernels():
    for t in TYPES:
        for op in ('p_add_mixed', 'p_add_mixed_nz', 'p_add', 'p_dbl', 'p_dbl_affine', 'p_neg_if', 'p_to_affine', 'p_mul_scalar', 'p_mul_affine_bits'):
            want = t.points and (op not in ('p_to_affine', 'p_mul_scalar', 'p_mul_affine_bits') or not t.lazy)
            assert (LIB.shape(t, op, 'straight') is not None) == want, (t, op)
    assert LIB.alt('p_add_mixed') == 'p_dbl' and LIB.alt('p_add') == 'p_dbl'


@pytest.mark.parametrize('op,mode', [('p_add_mixed', 'straight'), ('p_add_mixed', 'divergent'), ('p_add_mixed_nz', 'straight'),
                                     ('p_add', 'straight'), ('p_add', 'divergent')])
@pytest.mark.parametrize('t', POINT_TYPES, ids=str)
def test_point_addition(t, op, mode):
    """acc += q.  Divergent: lanes whose accumulator has an even first limb double it instead (curve.hpp dbl), as the lanes of an
    accumulation kernel take different branches."""
    assert LIB.shape(t, op, mode) == (8 if op == 'p_add' else 6, 4)
    run_points(t, op, mode, encode_pairs(t, op, 21 + t.id), group_expect(t))


@pytest.mark.parametrize('mode', ['straight', 'aliased'])
@pytest.mark.parametrize('t', POINT_TYPES, ids=str)
def test_point_dbl(t, mode):
    e = Enc(t, 31 + t.id)
    pts = base_points(t.fq2)
    cases = [(e.xyzz(pts[i % len(pts)]), pts[i % len(pts)], None, 'general') for i in range(N_GENERAL[t.fq2])]
    for lift in ((0, 1) if t.lazy else (0,)):
        cases += [(e.xyzz(None, lift, junk=j), None, None, 'infinity') for j in (False, True)]
        cases += [(e.xyzz(pts[i], lift), pts[i], None, 'wholly lifted %d' % lift) for i in range(4)]
    run_points(t, 'p_dbl', mode, cases, group_expect(t))


@pytest.mark.parametrize('t', POINT_TYPES, ids=str)
def test_point_dbl_affine(t):
    e = Enc(t, 41 + t.id)
    pts = base_points(t.fq2)
    cases = [(e.affine(pts[i % len(pts)]), pts[i % len(pts)], None, 'general') for i in range(N_GENERAL[t.fq2])]
    for lift in ((0, 1) if t.lazy else (0,)):
        cases += [(e.affine(pts[i], lift), pts[i], None, 'wholly lifted %d' % lift) for i in range(4)]
    run_points(t, 'p_dbl_affine', 'straight', cases, group_expect(t))


MUL_TYPES = [t for t in POINT_TYPES if not t.lazy]      # the product multiplies in Fq, FqC (G1) and Fq2, Fq2C (G2) only
R_ORDER = ref.R


def raw_el(t, k):
    """raw words in an element's place (csrc/fieldtest.hip): the first 8 words of the element"""
    return (k, 0) if t.fq2 else k


@pytest.mark.parametrize('t', MUL_TYPES, ids=str)
def test_point_mul_scalar(t):
    """Xyzz::mul_scalar(p, k) == k p for any 256-bit k.  k = r gives infinity: this call is the subgroup check of B in the verifiers
    (verify.hip, verify_agg.hip, keyfile.hip)."""
    assert LIB.shape(t, 'p_mul_scalar', 'straight') == (5, 4)
    G, _ = curve(t)
    e = Enc(t, 71 + t.id)
    pts, rnd = base_points(t.fq2), random.Random(72 + t.id)
    special = [0, 1, 2, 3, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 256) - 1, 1 << 255, 1 << 32, (1 << 32) - 1, 2 * R_ORDER]
    cases = []
    for i, k in enumerate(special):
        for j in range(2):
            pt = pts[(2 * i + j) % len(pts)]
            cases.append((e.xyzz(pt) + (raw_el(t, k),), pt, k, 'k = %#x' % k))
            cases.append(((e.el(pt[0]), e.el(pt[1]), e.el(e.F.one), e.el(e.F.one), raw_el(t, k)), pt, k, 'k = %#x, ZZ = ZZZ = 1' % k))
        cases.append((e.xyzz(None, junk=bool(i & 1)) + (raw_el(t, k),), None, k, 'infinity, k = %#x' % k))
    for i in range(24 if t.fq2 else 40):
        pt, k = pts[rnd.randrange(len(pts))], rnd.getrandbits(rnd.choice((256, 254, 128, 64)))
        cases.append((e.xyzz(pt) + (raw_el(t, k),), pt, k, 'random'))
    assert all(G.mul(p, R_ORDER) is None for p in pts[:4])
    run_points(t, 'p_mul_scalar', 'straight', cases, lambda which, a, k: G.mul(a, k))


@pytest.mark.parametrize('t', MUL_TYPES, ids=str)
def test_point_mul_affine_bits(t):
    """Xyzz::mul_affine_bits(p, lo, hi, nbits) == (hi 2^64 + lo) p: w A and w C of the aggregate verifier, the ceremony's random
    combinations.  The product calls it with nbits = 128 only; 64 is the other width its contract names (k below 2^nbits)."""
    assert LIB.shape(t, 'p_mul_affine_bits', 'straight') == (3, 4)
    G, _ = curve(t)
    e = Enc(t, 81 + t.id)
    pts, rnd = base_points(t.fq2), random.Random(82 + t.id)
    m64 = (1 << 64) - 1
    ks = [(1, 0, 128), (0, 1, 128), (m64, m64, 128), (0, 0, 128), (0, 1 << 63, 128), (m64, 0, 128), (2, 0, 128), (1, 0, 64), (m64, 0, 64), (1 << 63, 0, 64)]
    ks += [(rnd.getrandbits(64), rnd.getrandbits(64), 128) for _ in range(16 if t.fq2 else 30)] + [(rnd.getrandbits(64), 0, 64) for _ in range(4)]
    cases = []
    for i, (lo, hi, nbits) in enumerate(ks):
        pt, kel = pts[i % len(pts)], raw_el(t, lo | hi << 64 | nbits << 128)
        cases.append((e.affine(pt) + (kel,), pt, hi << 64 | lo, 'lo %#x hi %#x nbits %d' % (lo, hi, nbits)))
        if i < 10:
            cases.append((e.affine(None) + (kel,), None, hi << 64 | lo, 'infinity, lo %#x hi %#x nbits %d' % (lo, hi, nbits)))
    run_points(t, 'p_mul_affine_bits', 'straight', cases, lambda which, a, k: G.mul(a, k))


@pytest.mark.parametrize('t', POINT_TYPES, ids=str)
def test_affine_neg_if(t):
    """(x, y) -> (x, -y) when the flag is set, untouched otherwise; infinity (0, 0) stays infinity; y = 0 and, lazy, y = p"""
    G, F = curve(t)
    e = Enc(t, 51 + t.id)
    pts = base_points(t.fq2)
    flag = lambda b: (b, 0) if t.fq2 else b
    cases = []
    for i in range(N_GENERAL[t.fq2]):
        cases.append((e.affine(pts[i % len(pts)]) + (flag(i & 1),), 'general'))
    for b in (0, 1):
        for lift in ((0, 1) if t.lazy else (0,)):
            cases.append((e.affine(None, lift) + (flag(b),), 'infinity'))
            cases.append(((e.el(pts[0][0]), e.zero(lift), flag(b)), 'y = 0'))
    got = LIB.run(t, 'p_neg_if', 'straight', [c for c, _ in cases])
    bad = []
    for (c, lab), g in zip(cases, got):
        x, y, f = c
        neg = f[0] if t.fq2 else f
        if g[0] != x:
            why = 'x is not the very limbs that went in'
        elif neg:
            why = check_element(t, g[1], tuple(-v for v in y) if t.fq2 else -y)
        else:
            why = None if g[1] == y else 'y changed without the flag'
        if why:
            bad.append('[%s] %s: %s -> %s' % (lab, why, ' '.join(hexel(t, v) for v in c), ' '.join(hexel(t, v) for v in g)))
    print('%s p_neg_if straight: %d cases' % (t, len(cases)))
    assert not bad, '%d wrong\n%s' % (len(bad), '\n'.join(bad[:6]))


@pytest.mark.parametrize('t', [t for t in POINT_TYPES if not t.lazy], ids=str)
def test_to_affine(t):
    """canonical types: the affine Montgomery limbs are unique, so they are compared bit for bit; infinity gives the all-zero buffer"""
    G, F = curve(t)
    e = Enc(t, 61 + t.id)
    pts = base_points(t.fq2)
    n = N_GENERAL[t.fq2] // 2
    cases = [(e.xyzz(pts[i % len(pts)]), pts[i % len(pts)]) for i in range(n)] + [(e.xyzz(None, junk=j), None) for j in (False, True)]
    got = LIB.run(t, 'p_to_affine', 'straight', [c for c, _ in cases])
    bad = []
    for (c, pt), g in zip(cases, got):
        want = e.affine(pt)
        if tuple(g) != tuple(want):
            bad.append('%s -> %s, expected %s' % (' '.join(hexel(t, v) for v in c), ' '.join(hexel(t, v) for v in g), ' '.join(hexel(t, v) for v in want)))
    print('%s p_to_affine straight: %d cases' % (t, len(cases)))
    assert not bad, '%d wrong\n%s' % (len(bad), '\n'.join(bad[:6]))
