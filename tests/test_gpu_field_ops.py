"""The generated device field arithmetic (csrc/mont_mul_gfx950.inc, csrc/addsub_gfx950.inc) against Python integers.

Every proof byte passes through these inline-assembly carry chains, and only the device pass of field.hpp has them: the host pass,
the C oracle and the CPU tests run the plain C loops.  Here each method of Fp / Fq2T is called directly by a thin kernel of the
test-only library (csrc/fieldtest.hip) and compared with `(a * b * pow(2, -256, p)) % p` and the like -- not with the C oracle,
which shares the CIOS shape of `mul_body`.

Contract, asserted for EVERY case (none is skipped) and every result limb vector r of an operation whose exact value is v:
  canonical types (Fq, FqC, Fr, Fq2, Fq2C):  r == v mod p, bit for bit
  lazy types (FqL, FrL, Fq2T<FqL>):          r < 2p and r mod p == v mod p

Operands (lazy types draw from all of [0, 2p), both representatives x and x + p of a residue included):
  edges      E x E over a list E of ~40 values (0, 1, 2, p - 1, p, p + 1, 2p - 1, q - 1, R, R^2, 2^k and 2^k - 1, one saturated limb,
             0x80000000 in every limb; clipped below q); further operands of wider operations are rotations of E; for operations of
             two chains the two operand sets are also exchanged (cross-talk between chain 1 and chain 2)
  structured each limb from {0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff, uniform}, the top limb below q's
  targeted   products solved to come out at 0, 1, p - 1 (b = t R / a, lifted by p in lazy types); sums landing on q - 1, q, q + 1;
             differences of -1, 0, 1 and a = 0
  uniform    a few hundred, the common case
Random 254-bit operands reach none of the first three: a limb of 0 or 0xffffffff, a sum on q, a reduction ending at p.

inv, pow, pow_u64, from_u64 (and Fq2T::inv) are the loops everything above the field is built on (to_affine, the slopes of the Miller
loop, the final exponentiation): inv against a^-1 R^2 (0 -> 0, the Fermat value, pinned), pow against Python's pow.  The exponent
of pow, and the 64-bit argument of pow_u64 / from_u64, are raw words in an element's place, not range-limited (RAW).

Modes (csrc/fieldtest.hip): straight with a partial last wave; divergent (odd first operands run the operation, the others a
different one, both checked); aliased (outputs written over inputs by the call).

Known limit: the wrappers are separate kernels.  The assembly bodies are the same text as in msm_accumulate_kernel or
ntt_pass_kernel, the compiler's scheduling around them is not; the whole-MSM and whole-transform parity tests remain the check on
that.  This file closes the operand-space gap.
"""
import functools
import random

import pytest

from _fieldtest import MONT_R, TYPES, FieldTestLib, check_element, edge_list, first_limb_odd, hexel, structured

pytestmark = pytest.mark.gpu

LIB = FieldTestLib()        # the module-level guard: after one failed call nothing more is launched from this module

N_STRUCTURED, N_UNIFORM = 4000, 300


# ------------------------------------------------------------------------------------------------ the reference: exact values
def _lift(f):
    """a function of base-field integers -> the same on elements (componentwise for the pairs of an Fq2 type)"""
    def g(t, *a):
        if t.fq2:
            return tuple(f(t, *[x[i] for x in a]) for i in range(2))
        return f(t, *a)
    return g


add = _lift(lambda t, a, b: a + b)
sub = _lift(lambda t, a, b: a - b)
neg = _lift(lambda t, a: -a)


def mul(t, a, b):
    """the Montgomery product a b / 2^256"""
    if t.fq2:
        return ((a[0] * b[0] - a[1] * b[1]) * t.rinv, (a[0] * b[1] + a[1] * b[0]) * t.rinv)
    return a * b * t.rinv


def is_zero(t, a):
    return all(v % t.p == 0 for v in a) if t.fq2 else a % t.p == 0


def _inv(t, v):
    return pow(v, -1, t.p) if v % t.p else 0          # Fermat: 0^(p - 2) = 0


def inv(t, a):
    """the image of 1 / x for the image a of x: a^-1 R^2; in Fq2, conj(a) R^2 / (a0^2 + a1^2)"""
    if t.fq2:
        n = _inv(t, a[0] * a[0] + a[1] * a[1]) * MONT_R * MONT_R
        return (a[0] * n, -a[1] * n)
    return _inv(t, a) * MONT_R * MONT_R


def power(t, a, e):
    return pow(a * t.rinv % t.p, e, t.p) * MONT_R


U64 = (1 << 64) - 1


def flag(t, b):
    return (int(b), 0) if t.fq2 else int(b)


# name -> (operands, results, exact, function of (type, operands) returning the tuple of exact result values)
REF = {
    'add': (2, 1, False, lambda t, a: (add(t, a[0], a[1]),)),
    'sub': (2, 1, False, lambda t, a: (sub(t, a[0], a[1]),)),
    'dbl': (1, 1, False, lambda t, a: (add(t, a[0], a[0]),)),
    'neg': (1, 1, False, lambda t, a: (neg(t, a[0]),)),
    'add2': (4, 2, False, lambda t, a: (add(t, a[0], a[1]), add(t, a[2], a[3]))),
    'sub2': (4, 2, False, lambda t, a: (sub(t, a[0], a[1]), sub(t, a[2], a[3]))),
    'addsub2': (4, 2, False, lambda t, a: (add(t, a[0], a[1]), sub(t, a[2], a[3]))),
    'mul': (2, 1, False, lambda t, a: (mul(t, a[0], a[1]),)),
    'sqr': (1, 1, False, lambda t, a: (mul(t, a[0], a[0]),)),
    'mul2': (4, 2, False, lambda t, a: (mul(t, a[0], a[1]), mul(t, a[2], a[3]))),
    'sqr2': (2, 2, False, lambda t, a: (mul(t, a[0], a[0]), mul(t, a[1], a[1]))),
    'mulsub': (4, 1, False, lambda t, a: (sub(t, mul(t, a[0], a[1]), mul(t, a[2], a[3])),)),
    'dot4': (8, 1, False, lambda t, a: (sum(a[2 * i] * a[2 * i + 1] for i in range(4)) * t.rinv,)),
    'is_zero': (1, 1, True, lambda t, a: (flag(t, is_zero(t, a[0])),)),
    'eq': (2, 1, True, lambda t, a: (flag(t, is_zero(t, sub(t, a[0], a[1]))),)),
    'canon': (1, 1, True, lambda t, a: (a[0],)),                       # canon() then lazy_of(): the canonical limbs of the same residue
    'from_mont': (1, 1, False, lambda t, a: (a[0] * t.rinv,)),
    'to_mont': (1, 1, False, lambda t, a: (a[0] * MONT_R,)),
    'inv': (1, 1, False, lambda t, a: (inv(t, a[0]),)),
    'pow': (2, 1, False, lambda t, a: (power(t, a[0], a[1]),)),
    'pow_u64': (2, 1, False, lambda t, a: (power(t, a[0], a[1] & U64),)),
    'from_u64': (1, 1, False, lambda t, a: ((a[0] & U64) * MONT_R,)),
}
RAW = {'pow': (1,), 'pow_u64': (1,), 'from_u64': (0,)}       # operands that are raw words: any 256-bit value may stand there
FIELD_OPS = list(REF)


def has(t, op):
    """what field.hpp offers (the library must agree: test_library_offers_what_the_tests_expect)"""
    if op == 'dot4':
        return not t.lazy and not t.fq2
    if op == 'canon':
        return t.lazy
    if op in ('from_mont', 'to_mont', 'pow', 'pow_u64', 'from_u64'):        # Fq2T has none of these; Fq2T::inv it has
        return not t.fq2
    return True


DIVERGENT_ALT = {'add': 'mul', 'sub': 'add', 'dbl': 'neg', 'neg': 'sqr', 'mul': 'sub', 'sqr': 'dbl', 'add2': 'sqr2', 'sub2': 'add2',
                 'addsub2': 'mul2', 'mul2': 'addsub2', 'sqr2': 'sub2', 'mulsub': 'mul2', 'dot4': 'mulsub', 'from_mont': 'to_mont',
                 'to_mont': 'from_mont', 'inv': 'pow', 'pow': 'inv'}
ALIASED = ('add', 'sub', 'dbl', 'mul', 'sqr', 'mulsub', 'add2', 'sub2', 'addsub2', 'mul2', 'sqr2')


def modes_of(t, op):
    return ['straight'] + (['divergent'] if op in DIVERGENT_ALT and has(t, DIVERGENT_ALT[op]) else []) + (['aliased'] if op in ALIASED else [])


COMBOS = [(t, op, mode) for t in TYPES for op in FIELD_OPS if has(t, op) for mode in modes_of(t, op)]


# ------------------------------------------------------------------------------------------------ operands
def lifts(p, lazy, x):
    return [x, x + p] if lazy and x < p else [x]


@functools.lru_cache(maxsize=None)
def general_cases(p, lazy, k):
    """cases of k base-field operands: (operands, class) -- edges, structured, uniform"""
    q = 2 * p if lazy else p
    rnd = random.Random(1000 * k + 2 * (p & 0xffff) + lazy)
    e = edge_list(p, lazy)
    n = len(e)
    out = []
    if k == 1:
        out += [((x,), 'edges') for x in e]
    else:
        others = sorted({1, k // 2})        # E x E on operands (0, 1), and on (0, k/2): the first operands of the two halves
        for j in others:
            for ia, a in enumerate(e):
                for ib, b in enumerate(e):
                    ops = [e[(ia + 3 * ib + 7 * m) % n] for m in range(k)]
                    ops[0], ops[j] = a, b
                    out.append((tuple(ops), 'edges'))
                    if k >= 4 and j == 1:   # the two chains (halves) with exchanged operand sets
                        out.append((tuple(ops[k // 2:] + ops[:k // 2]), 'edges, chains exchanged'))
    out += [(tuple(structured(rnd, q) for _ in range(k)), 'structured') for _ in range(N_STRUCTURED)]
    out += [(tuple(rnd.randrange(q) for _ in range(k)), 'uniform') for _ in range(N_UNIFORM)]
    return tuple(out)


def _nonzero(rnd, p, q):
    while True:
        a = structured(rnd, q) if rnd.randrange(2) else rnd.randrange(q)
        if a % p:
            return a


@functools.lru_cache(maxsize=None)
def t_mul(p, lazy):
    """(a, b) with a b / R = t for t in 0, 1, p - 1: b = t R / a.  In a lazy type every representative of a and b, so that the
    unreduced product may end at p or p + 1 as well."""
    rnd, q, out = random.Random(11), 2 * p if lazy else p, []
    for t in (0, 1, p - 1):
        for _ in range(12):
            a = _nonzero(rnd, p, q)
            b = t * MONT_R * pow(a, -1, p) % p
            out += [(x, y) for x in lifts(p, lazy, a % p) for y in lifts(p, lazy, b)]
            out += [(y, x) for x in lifts(p, lazy, a % p) for y in lifts(p, lazy, b)][:1]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def t_mulsub(p, lazy):
    """(a, b, c, d) with (a b - c d) / R = t; and c = 0, whose negative as a product operand is q itself"""
    rnd, q, out = random.Random(12), 2 * p if lazy else p, []
    for t in (0, 1, p - 1):
        for _ in range(12):
            a, b, c = (_nonzero(rnd, p, q) for _ in range(3))
            d = (a * b - t * MONT_R) * pow(c, -1, p) % p
            out += [(a, b, c, y) for y in lifts(p, lazy, d)]
        for a, b in t_mul(p, lazy)[:8] if t == 0 else ():
            out += [(a, b, 0, _nonzero(rnd, p, q)), (a, b, _nonzero(rnd, p, q), 0)]
    for a, b in t_mul(p, lazy):
        out += [(a, b, z, _nonzero(rnd, p, q)) for z in lifts(p, lazy, 0)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def t_add(p, lazy):
    """(a, b) with a + b on and beside q (and, in a lazy type, p and 3p)"""
    rnd, q, out = random.Random(13), 2 * p if lazy else p, []
    for s in (q - 1, q, q + 1) + ((p - 1, p, p + 1, 3 * p - 1, 3 * p, 3 * p + 1) if lazy else ()):
        for i in range(12):
            lo, hi = max(0, s - (q - 1)), min(q - 1, s)
            a = (lo, hi, (lo + hi) // 2)[i] if i < 3 else rnd.randrange(lo, hi + 1)
            out.append((a, s - a))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def t_sub(p, lazy):
    """(a, b) with a - b in -1, 0, 1 (in a lazy type also beside p and -p), and a = 0"""
    rnd, q, out = random.Random(14), 2 * p if lazy else p, []
    for d in (-1, 0, 1) + ((p - 1, p, p + 1, -p - 1, -p, -p + 1) if lazy else ()):
        for i in range(12):
            lo, hi = max(0, d), min(q - 1, q - 1 + d)          # a in [lo, hi] keeps b = a - d in [0, q)
            a = (lo, hi)[i] if i < 2 else (structured(rnd, q) if i < 7 else rnd.randrange(q))
            a = min(max(a, lo), hi)
            out.append((a, a - d))
    out += [(0, b) for b in edge_list(p, lazy)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def t_dbl(p, lazy):
    q = 2 * p if lazy else p
    vals = [(p - 1) // 2, (p + 1) // 2, (q - 1) // 2, (q + 1) // 2, q // 2] + ([p + (p - 1) // 2, p + (p + 1) // 2, p - 1, p, p + 1] if lazy else [])
    return tuple((v,) for v in vals if v < q)


@functools.lru_cache(maxsize=None)
def t_inv(p, lazy):
    """images 0, 1, p - 1, R, 1 / 2, and those whose inverse's image is 1, p - 1 or R; in a lazy type both representatives"""
    r = MONT_R % p
    vals = [0, 1, p - 1, r, (p + 1) // 2, r * r % p, -r * r % p, (p + 1) // 2 * r % p]
    return tuple((y,) for x in vals for y in lifts(p, lazy, x))


@functools.lru_cache(maxsize=None)
def t_pow(p, lazy):
    """(a, e): e in 0, 1, 2, p - 2, (p - 1) / 2, 2^256 - 1, 2^255, and with zero high words; a = 0 among the bases"""
    rnd, q = random.Random(17), 2 * p if lazy else p
    es = [0, 1, 2, p - 2, (p - 1) // 2, (1 << 256) - 1, 1 << 255, p, 2 * p + 1] + [rnd.getrandbits(k) | 1 << (k - 1) for k in (31, 32, 33, 64, 96, 128, 224)]
    bases = [0, 1, p - 1, MONT_R % p] + [_nonzero(rnd, p, q) for _ in range(4)] + ([p, p + 1] if lazy else [])
    return tuple((a, e) for e in es for a in bases)


@functools.lru_cache(maxsize=None)
def t_pow_u64(p, lazy):
    """(a, e): e in 0, 1, 2^63, 2^64 - 1, alone and under words the method must not see"""
    rnd, q = random.Random(18), 2 * p if lazy else p
    es = [0, 1, 2, 1 << 63, U64, 1 << 32, (1 << 32) - 1]
    es += [e | rnd.getrandbits(192) << 64 for e in es]
    return tuple((a, e) for e in es for a in (0, MONT_R % p, _nonzero(rnd, p, q), _nonzero(rnd, p, q)))


def t_from_u64(p, lazy):
    return tuple((x | hi << 64,) for x in (0, 1, 1 << 32, U64, 1 << 63, (1 << 32) - 1) for hi in (0, 1, (1 << 192) - 1))


def _rot(xs, k):
    k %= len(xs)
    return xs[k:] + xs[:k]


def f2mul(p, a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def f2inv(p, a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, p)
    return (a[0] * n % p, -a[1] * n % p)


F2_TARGETS = lambda p: ((0, 0), (1, 0), (p - 1, 0), (0, 1), (0, p - 1), (1, p - 1), (p - 1, 1))


@functools.lru_cache(maxsize=None)
def t_fq2mul(p, lazy):
    """(a0, a1, b0, b1) with a b / R = T, each component of T in 0, 1, p - 1"""
    rnd, q, out = random.Random(15), 2 * p if lazy else p, []
    for tt in F2_TARGETS(p):
        for _ in range(6):
            a = (_nonzero(rnd, p, q), _nonzero(rnd, p, q))
            b = f2mul(p, (tt[0] * MONT_R % p, tt[1] * MONT_R % p), f2inv(p, a))
            for _ in range(3 if lazy else 1):
                out.append(a + tuple(rnd.choice(lifts(p, lazy, v)) for v in b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def t_fq2mulsub(p, lazy):
    """(a, b, c, d) as eight base operands with (a b - c d) / R = T; and c, d with zero components (their negatives are q)"""
    rnd, q, out = random.Random(16), 2 * p if lazy else p, []
    for tt in F2_TARGETS(p):
        for _ in range(6):
            a, b, c = ((_nonzero(rnd, p, q), _nonzero(rnd, p, q)) for _ in range(3))
            ab = f2mul(p, a, b)
            d = f2mul(p, ((ab[0] - tt[0] * MONT_R) % p, (ab[1] - tt[1] * MONT_R) % p), f2inv(p, c))
            for _ in range(3 if lazy else 1):
                out.append(a + b + c + tuple(rnd.choice(lifts(p, lazy, v)) for v in d))
    for m in t_fq2mul(p, lazy):
        for z in lifts(p, lazy, 0):
            out.append(m + (z, _nonzero(rnd, p, q), z, z))
            out.append(m + (_nonzero(rnd, p, q), z, _nonzero(rnd, p, q), z))
    return tuple(out)


def targeted(t, op):
    """cases of the operation's own operand count, as tuples of base-field operands"""
    p, lazy = t.p, t.lazy
    pair2 = lambda xs, ys: [x + y for x, y in zip(xs, _rot(ys, 5))] + [x + y for x, y in zip(_rot(ys, 3), xs)]
    if not t.fq2:
        base = {'add': t_add, 'sub': t_sub, 'eq': t_sub, 'dbl': t_dbl, 'mul': t_mul, 'mulsub': t_mulsub,
                'inv': t_inv, 'pow': t_pow, 'pow_u64': t_pow_u64, 'from_u64': t_from_u64}
        if op in base:
            return list(base[op](p, lazy))
        if op == 'add2':
            return pair2(t_add(p, lazy), t_add(p, lazy))
        if op == 'sub2':
            return pair2(t_sub(p, lazy), t_sub(p, lazy))
        if op == 'addsub2':
            return [x + y for x, y in zip(t_add(p, lazy), _rot(t_sub(p, lazy), 5))] + [x + y for x, y in zip(_rot(t_add(p, lazy), 3), t_sub(p, lazy))]
        if op == 'mul2':
            return pair2(t_mul(p, lazy), t_mul(p, lazy))
        return []
    # an Fq2 operand is (c0, c1): two base cases (x0, y0), (x1, y1) of a componentwise operation make one case (x0, x1, y0, y1)
    comp = lambda xs: [(x[0], y[0], x[1], y[1]) for x, y in zip(xs, _rot(xs, 7))] if len(xs[0]) == 2 else [(x[0], y[0]) for x, y in zip(xs, _rot(xs, 2))]
    if op in ('add', 'sub', 'eq', 'dbl'):
        return comp(list({'add': t_add, 'sub': t_sub, 'eq': t_sub, 'dbl': t_dbl}[op](p, lazy)))
    if op in ('add2', 'sub2', 'addsub2'):
        xs = comp(list((t_add if op != 'sub2' else t_sub)(p, lazy)))
        ys = comp(list((t_add if op == 'add2' else t_sub)(p, lazy)))
        return [x + y for x, y in zip(xs, _rot(ys, 5))] + [x + y for x, y in zip(_rot(xs, 3), ys)]
    if op == 'mul':
        return list(t_fq2mul(p, lazy))
    if op == 'mul2':
        return pair2(t_fq2mul(p, lazy), t_fq2mul(p, lazy))
    if op == 'mulsub':
        return list(t_fq2mulsub(p, lazy))
    if op == 'inv':         # norm zero only at 0; pure real, pure imaginary, and every pair of the base targets
        xs = [x for x, in t_inv(p, lazy)]
        return [(x, y) for x in xs for y in xs]
    return []


def cases_for(t, op, operands):
    """(list of cases as tuples of `operands` elements, list of their classes).  `operands` may exceed the operation's own count
    (divergent mode with a wider other arm): the further operands are edge values."""
    k = operands * t.w
    gen = general_cases(t.p, t.lazy, k)
    flat, labels = [c for c, _ in gen], [l for _, l in gen]
    e = edge_list(t.p, t.lazy)
    for i, c in enumerate(targeted(t, op)):
        assert len(c) == REF[op][0] * t.w and all(0 <= v < (MONT_R if j in RAW.get(op, ()) else t.q) for j, v in enumerate(c)), (op, c)
        flat.append(tuple(c) + tuple(e[(i + 5 * m) % len(e)] for m in range(k - len(c))))
        labels.append('targeted')
    if len(flat) % 64 == 0:         # the last wave is partial
        flat.append(flat[-1])
        labels.append(labels[-1])
    if t.fq2:
        return [tuple(zip(c[0::2], c[1::2])) for c in flat], labels
    return flat, labels


# ------------------------------------------------------------------------------------------------ the tests
def test_library_offers_what_the_tests_expect():
    """the combinations this file runs are exactly the field kernels the library has: nothing is quietly left out on either side"""
    for t in TYPES:
        for op in FIELD_OPS:
            for mode in ('straight', 'divergent', 'aliased'):
                assert (LIB.shape(t, op, mode) is not None) == ((t, op, mode) in COMBOS), (t, op, mode)
    for op, alt in DIVERGENT_ALT.items():
        assert LIB.alt(op) == alt


@pytest.mark.parametrize('t,op,mode', COMBOS, ids=['%s-%s-%s' % c for c in COMBOS])
def test_field_op(t, op, mode):
    ni, no = LIB.shape(t, op, mode)
    alt = DIVERGENT_ALT[op] if mode == 'divergent' else op
    assert (ni, no) == (max(REF[op][0], REF[alt][0]), max(REF[op][1], REF[alt][1]))
    cases, labels = cases_for(t, op, ni)
    got = LIB.run(t, op, mode, cases)
    zero = (0, 0) if t.fq2 else 0
    bad, arms = [], {op: 0, alt: 0}
    for c, lab, g in zip(cases, labels, got):
        which = op if mode != 'divergent' or first_limb_odd(t, c[0]) else alt
        arms[which] += 1
        nin, nout, exact, fn = REF[which]
        want = fn(t, c[:nin])
        for j in range(no):
            why = check_element(t, g[j], want[j], exact) if j < nout else (None if g[j] == zero else 'a result the operation does not have was written')
            if why:
                bad.append('%s [%s] result %d %s: operands %s -> got %s, exact value mod p %s'
                           % (which, lab, j, why, ' '.join(hexel(t, x) for x in c[:nin]), hexel(t, g[j]),
                              hexel(t, tuple(v % t.p for v in want[j]) if t.fq2 else want[j] % t.p)))
    print('%s %s %s: %d cases (%s)' % (t, op, mode, len(cases), ', '.join('%s %d' % kv for kv in arms.items())))
    if mode == 'divergent':
        assert min(arms.values()) > len(cases) // 8, 'divergent mode needs lanes in both arms: %r' % arms
    assert not bad, '%d of %d results wrong; by class: %s\n%s' % (
        len(bad), len(cases) * no, sorted({b.split(']')[0].split('[')[1] for b in bad}), '\n'.join(bad[:8]))
