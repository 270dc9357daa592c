"""Case lists and checks shared by test_tower_host.py (where = 'host': Fq, the type fk_verify uses, no GPU) and test_gpu_tower_ops.py
(where = 'device': FqC, one lane per case).  Both run the same cases through the thin wrappers of csrc/fieldtest_tower.hip and compare
with _tower_ref.py.

Contract: every result limb image equals the exact value mod p, bit for bit, for every case; no case is skipped or filtered.

What goes to the library is Montgomery limb images (the tests choose the limbs: 0, 1, p - 1, R, R^2, saturated limbs, from the
generators of _fieldtest.py); the reference works on the values they stand for (image / 2^256) and its result is brought back to an
image.  Expected values are computed once per process and shared by the two test files.
"""
import functools
import random

import bn254_ref as ref
import _tower_ref as tr
from _fieldtest import MONT_R, edge_list, structured

P = tr.P
EDGES = edge_list(P, False)
ONE_M = MONT_R % P                      # the Montgomery image of 1
N_UNARY, N_BINARY = 203, 331            # cases per operation, about; never a multiple of 64 (odd_count)


def blob(parts):
    return b''.join(v.to_bytes(32, 'little') for part in parts for v in part)


def unblob(b):
    return [int.from_bytes(b[i:i + 32], 'little') for i in range(0, len(b), 32)]


def coef(rnd, nonzero=False):
    """one base coefficient as a limb image: an edge value, a structured one or a uniform one"""
    while True:
        k = rnd.randrange(3)
        v = EDGES[rnd.randrange(len(EDGES))] if k == 0 else structured(rnd, P) if k == 1 else rnd.randrange(P)
        if v or not nonzero:
            return v


def rand_el(rnd, n):
    return [coef(rnd) for _ in range(n)]


def filled(rnd, n, positions):
    e = [0] * n
    for t in positions:
        e[t] = coef(rnd, nonzero=True)
    return e


def unit(n, t, image=ONE_M):
    e = [0] * n
    e[t] = image
    return e


def structured12(rnd):
    """Fq12 elements with structure, as (images, label): positions are those of the limb image, c0.c0.c0, c0.c0.c1, c0.c1.c0, ..."""
    out = [([0] * 12, 'zero'), (unit(12, 0), 'one'),
           (filled(rnd, 12, [0]), 'in Fq'), (filled(rnd, 12, [0, 1]), 'in Fq2'), (filled(rnd, 12, range(6)), 'in Fq6 (c1 = 0)'),
           (filled(rnd, 12, range(6, 12)), 'c0 = 0'),
           (unit(12, 2), 'v'), (unit(12, 6), 'w'), (unit(12, 8), 'w^3'), (unit(12, 0, 9 * ONE_M % P)[:1] + [ONE_M] + [0] * 10, 'xi')]
    out += [(filled(rnd, 12, [t, t + 1]), 'only the Fq2 coefficient at position %d' % (t // 2)) for t in range(0, 12, 2)]
    return out


def structured6(rnd):
    out = [([0] * 6, 'zero'), (unit(6, 0), 'one'), (filled(rnd, 6, [0]), 'in Fq'), (filled(rnd, 6, [0, 1]), 'in Fq2'),
           (unit(6, 2), 'v'), (unit(6, 4), 'v^2'), ([9 * ONE_M % P, ONE_M, 0, 0, 0, 0], 'xi')]
    out += [(filled(rnd, 6, [t, t + 1]), 'only c%d' % (t // 2)) for t in range(0, 6, 2)]
    return out


def structured2(rnd):
    return [([0, 0], 'zero'), ([ONE_M, 0], 'one'), ([0, ONE_M], 'u'), ([9 * ONE_M % P, ONE_M], 'xi'), ([P - 1, P - 1], 'p - 1 twice'),
            (filled(rnd, 2, [0]), 'real'), (filled(rnd, 2, [1]), 'imaginary')]


STRUCTURED = {12: structured12, 6: structured6, 2: structured2}


def unary(rnd, n, count=N_UNARY):
    """`count` elements of n base coefficients: three draws of every structured element, then random ones"""
    out = [c for _ in range(3) for c in STRUCTURED[n](rnd)]
    while len(out) < count:
        out.append((rand_el(rnd, n), 'random'))
    return out


def binary(rnd, n, m, count=N_BINARY):
    """pairs (a of n coefficients, b of m): every structured element in each position against a random one, structured against
    structured, random against random"""
    sa, sb, out = STRUCTURED[n](rnd), STRUCTURED[m](rnd), []
    for _ in range(2):
        out += [((a, rand_el(rnd, m)), la + ' x random') for a, la in STRUCTURED[n](rnd)]
        out += [((rand_el(rnd, n), b), 'random x ' + lb) for b, lb in STRUCTURED[m](rnd)]
    for i, (a, la) in enumerate(sa):
        for k in (0, 1, 5):
            b, lb = sb[(i + k) % len(sb)]
            out.append(((a, b), la + ' x ' + lb))
    while len(out) < count:
        out.append(((rand_el(rnd, n), rand_el(rnd, m)), 'random x random'))
    return out


def odd_count(cases):
    """the last wave is partial"""
    return cases + cases[-1:] if len(cases) % 64 == 0 else cases


# ------------------------------------------------------------------------------------------------ the reference, on values
def mul12(a, b):
    return tr.from_poly(ref.f12_mul(tr.to_poly(a), tr.to_poly(b)))


def inv12(a):
    """0 -> 0: what the Fermat inversion at the bottom of the tower returns, pinned here"""
    return [0] * 12 if not any(a) else tr.from_poly(ref.f12_inv(tr.to_poly(a)))


def low(x, n):
    assert not any(x[n:]), 'the reference result left the subfield'
    return x[:n]


e6, e2 = tr.f6_embed, tr.f2_embed
V12, XI12 = unit(12, 2, 1), [9, 1] + [0] * 10
ARITH = {
    # name: (base coefficients of each operand, function of the operands' values -> the result's values)
    'f6_mul': ((6, 6), lambda a, b: low(mul12(e6(a), e6(b)), 6)),
    'f6_mul_by_01': ((6, 2, 2), lambda a, b0, b1: low(mul12(e6(a), e6(b0 + b1 + [0, 0])), 6)),
    'f6_mul_by_fq2': ((6, 2), lambda a, b: low(mul12(e6(a), e2(b)), 6)),
    'f6_mul_v': ((6,), lambda a: low(mul12(e6(a), V12), 6)),
    'f6_mul_xi': ((2,), lambda a: low(mul12(e2(a), XI12), 2)),
    'f6_inv': ((6,), lambda a: low(inv12(e6(a)), 6)),
    'f6_add': ((6, 6), lambda a, b: [(x + y) % P for x, y in zip(a, b)]),
    'f6_sub': ((6, 6), lambda a, b: [(x - y) % P for x, y in zip(a, b)]),
    'f6_neg': ((6,), lambda a: [-x % P for x in a]),
    'f12_mul': ((12, 12), mul12),
    'f12_sqr_complex': ((12,), lambda a: mul12(a, a)),
    'f12_mul_by_line': ((12, 2, 2, 2), lambda a, l0, l1, l3: tr.from_poly(ref.f12_mul(tr.to_poly(a), tr.w_coeffs({0: l0, 1: l1, 3: l3})))),
    # a^(p^6) is the automorphism w -> -w (it fixes Fq6 = Fq(w^2)): the odd coefficients change sign.  test_tower_host.py holds
    # this against f12_pow(a, p^6)
    'f12_conj': ((12,), lambda a: tr.from_poly([-c % P if k & 1 else c for k, c in enumerate(tr.to_poly(a))])),
    'f12_inv': ((12,), inv12),
}


def _inverse_pairs(rnd, n, count):
    """(a, 1 / a) from f12_inv: products that come out at one"""
    out = []
    for i in range(count):
        a = filled(rnd, n, range(n)) if i else filled(rnd, n, range(min(n, 2)))
        ai = low(inv12(tr.mont_decode(a) + [0] * (12 - n)), n)
        out.append(((a, tr.mont_encode(ai)), 'b = 1 / a'))
    return out


def _sparse_operands(rnd, k):
    """the k Fq2 operands of a sparse product: each zero in turn, all zero, all but one zero, ones, structured, random"""
    z, out = [0, 0], []
    for i in range(k):
        out.append([z if j == i else rand_el(rnd, 2) for j in range(k)])
        out.append([rand_el(rnd, 2) if j == i else z for j in range(k)])
    out.append([z] * k)
    out.append([[ONE_M, 0]] * k)
    out += [[s] + [rand_el(rnd, 2) for _ in range(k - 1)] for s, _ in structured2(rnd)]
    out += [[rand_el(rnd, 2) for _ in range(k)] for _ in range(4)]
    return out


def _arith_operands(op):
    rnd = random.Random('tower ' + op)
    shape = ARITH[op][0]
    if op in ('f6_mul_by_01', 'f12_mul_by_line'):
        sparse = _sparse_operands(rnd, len(shape) - 1)
        els = unary(rnd, shape[0], 60)
        out = [((a,) + tuple(sparse[(i + 3 * j) % len(sparse)]), la + ', sparse operand %d' % ((i + 3 * j) % len(sparse)))
               for i, (a, la) in enumerate(els) for j in range(5)]
        out += [((rand_el(rnd, shape[0]),) + tuple(s), 'random, sparse operand %d' % i) for i, s in enumerate(sparse)]
    elif len(shape) == 1:
        out = [((a,), la) for a, la in unary(rnd, shape[0])]
    else:
        out = binary(rnd, shape[0], shape[1])
    if op in ('f6_mul', 'f12_mul'):
        out += _inverse_pairs(rnd, shape[0], 6)
    return odd_count(out)


@functools.lru_cache(maxsize=None)
def arith_cases(op):
    """(cases as (operands, label), expected images): computed once"""
    cases = _arith_operands(op)
    fn = ARITH[op][1]
    want = [tr.mont_encode(fn(*[tr.mont_decode(x) for x in ops])) for ops, _ in cases]
    if op in ('f6_mul', 'f12_mul'):
        n = ARITH[op][0][0]
        assert all(w == unit(n, 0) for (_, lab), w in zip(cases, want) if lab == 'b = 1 / a')
    return cases, want


def report(op, where, cases, bad):
    print('%s on the %s: %d cases' % (op, where, len(cases)))
    assert not bad, '%d of %d cases wrong; by class: %s\n%s' % (len(bad), len(cases), sorted({b.split(']')[0] for b in bad})[:12], '\n'.join(bad[:4]))


def hexes(xs):
    return ' '.join('%#x' % x for x in xs)


def check_arith(lib, where, op):
    cases, want = arith_cases(op)
    got = lib.run_tower(op, where, [blob(ops) for ops, _ in cases])
    bad = ['%s] operands %s -> %s, exact value %s' % (lab, ' | '.join(hexes(x) for x in ops), hexes(unblob(g)), hexes(w))
           for (ops, lab), g, w in zip(cases, got, want) if unblob(g) != w]
    report(op, where, cases, bad)


ARITH_OPS = list(ARITH)


# ------------------------------------------------------------------------------------------------ is_one
@functools.lru_cache(maxsize=None)
def is_one_cases():
    """(images, expected, label).  True on exactly the Montgomery one; every single coefficient, and every single limb, can alone
    make it false."""
    one = unit(12, 0)
    out = [(one, True, 'one'), ([0] * 12, False, 'zero'), (unit(12, 0, 1), False, 'the raw integer 1'), (unit(12, 0, P - ONE_M), False, '-1')]
    for t in range(12):
        for d, what in ((1, '+ 1'), (-1, '- 1')):
            e = list(one)
            e[t] = (e[t] + d) % P
            out.append((e, False, 'one with coefficient %d %s' % (t, what)))
        e = list(one)
        e[t] = P - 1
        out.append((e, False, 'one with coefficient %d = p - 1' % t))
        for k in range(8):
            e = list(one)
            e[t] ^= 1 << (32 * k)
            assert e[t] < P
            out.append((e, False, 'one with limb %d of coefficient %d changed' % (k, t)))
        out.append((one, True, 'one'))          # true lanes among the false ones
    assert all((e == one) == w for e, w, _ in out)
    return odd_count(out)


def check_is_one(lib, where):
    cases = is_one_cases()
    got = lib.run_tower('f12_is_one', where, [blob([e]) for e, _, _ in cases])
    bad = ['%s] is_one(%s) -> %s' % (lab, hexes(e), g.hex()) for (e, w, lab), g in zip(cases, got) if g != int(w).to_bytes(4, 'little')]
    report('f12_is_one', where, cases, bad)


# ------------------------------------------------------------------------------------------------ pow
POW_NWORDS = (1, 8, 16, 24)


def fexp_constants():
    return tr.words_value(tr.product_words('FK_FEXP_P2_PLUS_1')), tr.words_value(tr.product_words('FK_FEXP_HARD'))


@functools.lru_cache(maxsize=None)
def pow_cases():
    """(base images, exponent as stored (24 words), nwords, expected images, label).  pow reads `nwords` words: what lies above
    them is in the buffer and must be ignored."""
    rnd = random.Random('tower pow')
    p2p1, hard = fexp_constants()
    plan = []
    for n in POW_NWORDS:
        bits = 32 * n
        es = [(0, '0'), (1, '1'), (1 << (bits - 1), 'the top bit alone'), ((1 << bits) - 1, 'all ones'), ((1 << (bits - 32)) | 1, 'top word 1'),
              (rnd.getrandbits(bits), 'random')]
        es += [(1 << k, '2^%d' % k) for k in (31, 32, 33, 63, 64, 255, 256, 511, 512) if k < bits]
        es += [(1 << k, '2^%d, above the words read' % k) for k in (bits, bits + 31) if k < 768]
        if n > 1:
            es += [(rnd.getrandbits(bits - 32), 'leading zero word'), (rnd.getrandbits(31) | 1 << 31, 'all but the lowest word zero'),
                   ((1 << (bits - 32)) - 1, 'all ones under a zero word')]
        if n == 16:
            es.append((p2p1, 'FK_FEXP_P2_PLUS_1'))
        if n == 24:
            es += [(p2p1, 'FK_FEXP_P2_PLUS_1 in 24 words'), (hard, 'FK_FEXP_HARD')]
        plan += [(n, e, lab) for e, lab in es]
    bases = [rand_el(rnd, 12) for _ in range(3)] + [filled(rnd, 12, range(6)), unit(12, 0), [0] * 12]
    out = []
    for i, (n, e, lab) in enumerate(plan):
        a = bases[i % 3] if i % 11 else bases[3 + (i // 11) % 3]
        eff = e & ((1 << (32 * n)) - 1)
        want = tr.mont_encode(tr.from_poly(ref.f12_pow(tr.to_poly(tr.mont_decode(a)), eff)))
        if eff == 0:
            assert want == unit(12, 0)
        out.append((a, e, n, want, 'nwords %d, %s' % (n, lab)))
    return odd_count(out)


def check_pow(lib, where):
    cases = pow_cases()
    got = lib.run_tower('f12_pow', where, [blob([a]) + e.to_bytes(96, 'little') + n.to_bytes(4, 'little') for a, e, n, _, _ in cases])
    bad = ['%s] %s ^ %#x -> %s, exact value %s' % (lab, hexes(a), e, hexes(unblob(g)), hexes(w)) for (a, e, n, w, lab), g in zip(cases, got) if unblob(g) != w]
    report('f12_pow', where, cases, bad)


# ------------------------------------------------------------------------------------------------ final exponentiation
@functools.lru_cache(maxsize=None)
def final_exp_cases():
    """(images, expected images, label): random elements against f12_pow(f, (p^12 - 1) / r); elements of the proper subfields, which
    it must send to one (what miller_loop_proj rests on: pairing.hpp)"""
    rnd = random.Random('tower final exponentiation')
    one = unit(12, 0)
    out = []
    for i in range(4):
        a = [rnd.randrange(P) for _ in range(12)] if i else rand_el(rnd, 12)
        out.append((a, tr.mont_encode(tr.from_poly(ref.f12_pow(tr.to_poly(tr.mont_decode(a)), tr.FINAL_EXPONENT))), 'random'))
    for _ in range(3):
        out += [(filled(rnd, 12, [0]), one, 'in Fq'), (filled(rnd, 12, [0, 1]), one, 'in Fq2'), (filled(rnd, 12, [1]), one, 'in Fq2, imaginary'),
                (filled(rnd, 12, range(6)), one, 'in Fq6'), (filled(rnd, 12, [2, 3]), one, 'in Fq6, only c1')]
    out += [(one, one, 'one'), (unit(12, 0, P - ONE_M), one, '-1')]
    lanes = list(out)
    while len(lanes) < 70:                      # a partial second wave of repeats
        lanes.append(out[rnd.randrange(len(out))])
    return lanes


def check_final_exp(lib, where):
    cases = final_exp_cases()
    got = lib.run_tower('final_exp', where, [blob([a]) for a, _, _ in cases])
    bad = ['%s] %s -> %s, exact value %s' % (lab, hexes(a), hexes(unblob(g)), hexes(w)) for (a, w, lab), g in zip(cases, got) if unblob(g) != w]
    report('final_exp', where, cases, bad)
    for (a, w, lab), g in zip(cases[:4], got):  # the random ones: the result has order dividing r
        assert ref.f12_pow(tr.to_poly(tr.mont_decode(unblob(g))), tr.R_ORDER) == tr.ONE


# ------------------------------------------------------------------------------------------------ Miller loops
N_LANES = 66


@functools.lru_cache(maxsize=None)
def pairing_refs():
    """the distinct (P, Q) pairs and, once per pair, what the reference says:
    (P, Q, a b mod r or None for a pair with a point at infinity, f of the lines loop, final_exp of the _linefunc loop, label)"""
    rnd = random.Random('tower pairs')
    ks = (1, 2, tr.R_ORDER - 1, rnd.randrange(3, tr.R_ORDER - 1))
    out = []
    for a in ks:
        for b in ks:
            Pt, Qt = ref.G1.mul(ref.G1_GEN, a), ref.G2.mul(ref.G2_GEN, b)
            f = tr.miller_loop_lines(Pt, Qt)
            e = ref.final_exp(tr.miller_loop_linefunc(Pt, Qt))
            out.append((Pt, Qt, a * b % tr.R_ORDER, f, e, '%s G1, %s G2' % tuple('r - 1' if k == tr.R_ORDER - 1 else k for k in (a, b))))
    g1, g2 = ref.G1.mul(ref.G1_GEN, ks[3]), ref.G2.mul(ref.G2_GEN, ks[3])
    out += [(None, g2, None, tr.ONE, tr.ONE, 'P at infinity'), (g1, None, None, tr.ONE, tr.ONE, 'Q at infinity'),
            (None, None, None, tr.ONE, tr.ONE, 'both at infinity')]
    return out


def pair_blob(Pt, Qt):
    p = [0, 0] if Pt is None else tr.mont_encode(Pt)
    q = [0, 0, 0, 0] if Qt is None else tr.mont_encode([Qt[0][0], Qt[0][1], Qt[1][0], Qt[1][1]])
    return blob([p, q])


@functools.lru_cache(maxsize=None)
def lanes():
    """66 lanes, a partial second wave: every distinct pair once, the three with a point at infinity among the real ones (those lanes
    return early beside lanes that run the loop), then repeats in shuffled order"""
    n = len(pairing_refs())
    rnd = random.Random('tower lanes')
    order = list(range(n))
    rnd.shuffle(order)
    order += [rnd.randrange(n) for _ in range(N_LANES - n)]
    assert len(order) == N_LANES and len(set(order[:64])) >= 16 and {n - 3, n - 2, n - 1} <= set(order[:64])
    return order


class Pairings:
    """the four runs the Miller-loop tests look at, made once per library and place"""

    def __init__(self, lib, where):
        refs, order = pairing_refs(), lanes()
        blobs = [pair_blob(refs[i][0], refs[i][1]) for i in order]
        self.miller = lib.run_tower('miller_loop', where, blobs)
        self.proj = lib.run_tower('miller_loop_proj', where, blobs)
        self.fe = lib.run_tower('final_exp', where, self.miller)
        self.fe_proj = lib.run_tower('final_exp', where, self.proj)


def poly_of(b):
    return tr.to_poly(tr.mont_decode(unblob(b)))


def image_of(poly):
    return blob([tr.mont_encode(tr.from_poly(poly))])


def check_miller_value(pr):
    """miller_loop equals the reference loop exactly, in every lane"""
    refs, order = pairing_refs(), lanes()
    bad = ['%s] lane %d' % (refs[i][5], lane) for lane, i in enumerate(order) if pr.miller[lane] != image_of(refs[i][3])]
    assert not bad, bad


def check_proj_ratio(pr):
    """miller_loop_proj / miller_loop is a nonzero element of Fq2: zero at every polynomial index but 0 and 6"""
    refs, order = pairing_refs(), lanes()
    first, bad = {}, []
    for lane, i in enumerate(order):
        if i in first:
            if pr.proj[lane] != pr.proj[first[i]]:
                bad.append('%s] lane %d differs from lane %d of the same pair' % (refs[i][5], lane, first[i]))
            continue
        first[i] = lane
        ratio = ref.f12_mul(poly_of(pr.proj[lane]), ref.f12_inv(refs[i][3]))
        if any(c for k, c in enumerate(ratio) if k not in (0, 6)) or not (ratio[0] or ratio[6]):
            bad.append('%s] lane %d: the ratio is %s' % (refs[i][5], lane, ratio))
        if refs[i][2] is None and pr.proj[lane] != image_of(tr.ONE):
            bad.append('%s] lane %d: not one' % (refs[i][5], lane))
    assert not bad, bad


def check_pairing_value(pr):
    """final_exponentiation(miller_loop) equals final_exp of the oracle's own loop and e(G1, G2)^(a b); miller_loop_proj agrees with
    miller_loop after the final exponentiation, exactly"""
    refs, order = pairing_refs(), lanes()
    e11 = refs[0][4]
    assert refs[0][2] == 1 and e11 != tr.ONE and ref.f12_pow(e11, tr.R_ORDER) == tr.ONE
    power = {i: ref.f12_pow(e11, r[2]) if r[2] is not None else tr.ONE for i, r in enumerate(refs)}
    bad = []
    for lane, i in enumerate(order):
        want = image_of(refs[i][4])
        if refs[i][4] != power[i]:
            bad.append('%s] the reference itself is not bilinear' % refs[i][5])
        if pr.fe[lane] != want:
            bad.append('%s] lane %d: final_exponentiation(miller_loop) is not the pairing' % (refs[i][5], lane))
        if pr.fe_proj[lane] != pr.fe[lane]:
            bad.append('%s] lane %d: the two loops differ after the final exponentiation' % (refs[i][5], lane))
    assert not bad, bad
