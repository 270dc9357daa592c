"""Device JubJub and EdDSA-Poseidon (csrc/eddsa.hip) against the Python restatement of native/ecc.rs and native/eddsaposeidon.rs in
oracle/fawkes_circuit.py: scalar multiplication, subgroup decompression, verification and signing.  Every comparison is exact integer
equality.  Each reference list is computed once for the largest batch; the batches n = 1, 63, 64, 65 (a partial wave on either side of a
full one) and 129 (a partial second wave after two full ones) are its prefixes."""
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc

pytestmark = pytest.mark.gpu

R, FS = ref.R, fc.FS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eddsa_golden.json')
SIZES = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def curve():
    return fc.JubJubBN256()


@functools.lru_cache(maxsize=None)
def oracle_params():
    return fc.PoseidonParams(4, 8, 54)


@functools.lru_cache(maxsize=None)
def device_params():
    import fawkes_crypto_amd as fk
    return fk.PoseidonParams(4, 8, 54)


def has_root(x):
    x2 = x * x % R
    return fc.fr_sqrt((x2 + 1) * fc.fr_inv(1 - curve().d * x2) % R) is not None


@functools.lru_cache(maxsize=None)
def special_xs():
    """(an x whose y exists but whose point lies outside the prime subgroup, an x without a root), found with the oracle"""
    rnd = random.Random(4242)
    outside = rootless = None
    while outside is None or rootless is None:
        x = rnd.randrange(R)
        if not has_root(x):
            rootless = x if rootless is None else rootless
        elif outside is None and curve().subgroup_decompress(x) is None:
            outside = x
    return outside, rootless


def outside_point():
    x = special_xs()[0]
    x2 = x * x % R
    return (x, fc.fr_sqrt((x2 + 1) * fc.fr_inv(1 - curve().d * x2) % R))


# ---------------------------------------------------------------------------------------------- mul
@functools.lru_cache(maxsize=None)
def mul_cases():
    """129 (point, scalar) pairs and jj.mul of each: every edge point meets every edge scalar at least once, seeded random values fill up"""
    jj, rnd = curve(), random.Random(911)
    g = jj.g
    points = [(0, 1), (0, R - 1), g, ((R - g[0]) % R, g[1]), jj.mul(g, 2), jj.mul(g, 77), jj.mul(g, FS - 1), jj.mul(g, rnd.randrange(FS)), outside_point()]
    scalars = [0, 1, 2, 8, FS - 1, FS, FS + 1, 1 << 251, (1 << 256) - 1]
    pairs = [(points[(i + j) % len(points)], s) for j in range(len(points)) for i, s in enumerate(scalars)]
    rnd.shuffle(pairs)
    pairs = [(g, 1)] + pairs[:100]
    while len(pairs) < 129:
        pairs.append((rnd.choice(points), rnd.randrange(1 << 256)))
    assert {s for _, s in pairs} >= set(scalars) and {p for p, _ in pairs} == set(points)
    return tuple(pairs), tuple(jj.mul(p, k) for p, k in pairs)


def test_mul_matches_oracle(ctx):
    pairs, want = mul_cases()
    for n in SIZES:
        assert ctx.jubjub_mul([p for p, _ in pairs[:n]], [k for _, k in pairs[:n]]) == list(want[:n]), n
    assert ctx.jubjub_mul([], []) == []


def test_mul_generator_matches_oracle(ctx):
    """points=None means the generator"""
    from fawkes_crypto_amd import api
    jj, rnd = curve(), random.Random(912)
    scalars = [0, 1, 2, 8, FS - 1, FS, FS + 1, 1 << 251, (1 << 256) - 1] + [rnd.randrange(1 << 256) for _ in range(56)]
    want = [jj.mul(jj.g, k) for k in scalars]
    for n in (1, 63, 64, 65):
        assert ctx.jubjub_mul(None, scalars[:n]) == want[:n], n
    limbs = ctx.jubjub_mul(None, api._u256_rows(scalars[:5]))                 # limb arrays in, limbs out
    assert limbs.dtype == np.uint64 and limbs.shape == (5, 2, 4)
    assert api._fr_ints(limbs) == [c for pt in want[:5] for c in pt]


# ---------------------------------------------------------------------------------------------- decompress
@functools.lru_cache(maxsize=None)
def decompress_cases():
    jj, rnd = curve(), random.Random(777)
    g = jj.g
    outside, _ = special_xs()
    xs = [0, 1, R - 1, g[0], R - g[0], outside, R - outside]
    for _ in range(29):
        x = jj.mul(g, rnd.randrange(1, FS))[0]
        xs += [x, R - x]
    xs += [rnd.randrange(R) for _ in range(64)]
    assert len(xs) == 129
    want = tuple(jj.subgroup_decompress(x) for x in xs)
    return tuple(xs), want


def test_decompress_matches_oracle(ctx):
    xs, want = decompress_cases()
    # what the oracle's answers must cover: the three outcomes, and accepted points of both signs of x (so that both branches of the
    # final sign choice run whichever root the device takes)
    no_root = sum(1 for x in xs if not has_root(x))
    outside = sum(1 for x, w in zip(xs, want) if w is None and has_root(x))
    accepted = [x for x, w in zip(xs, want) if w is not None]
    assert no_root >= 8 and outside >= 8 and len(accepted) >= 8, (no_root, outside, len(accepted))
    assert any(x != 0 and R - x in accepted for x in accepted)
    ys = [None if w is None else w[1] for w in want]
    for n in SIZES:
        assert ctx.jubjub_decompress(list(xs[:n])) == ys[:n], n
    assert ctx.jubjub_decompress([]) == []


# ---------------------------------------------------------------------------------------------- verify
@functools.lru_cache(maxsize=None)
def verify_cases():
    """129 rows (s, r, a, m, expected): valid signatures, the corruptions the oracle judges, and the rows the ABI rejects by rule.
    m_is_r marks the rows whose m is to be passed as the limb image of r itself."""
    jj, pp, rnd = curve(), oracle_params(), random.Random(1337)
    outside, rootless = special_xs()
    keys = [(1, rnd.randrange(R), rnd.randrange(FS)), (0, rnd.randrange(R), rnd.randrange(FS)), (rnd.randrange(FS), rnd.randrange(R), 0),
            (rnd.randrange(FS), 0, rnd.randrange(FS)), (rnd.randrange(FS), R - 1, rnd.randrange(FS))]
    while len(keys) < 48:
        keys.append((rnd.randrange(FS), rnd.randrange(R), rnd.randrange(FS)))
    valid = [fc.eddsaposeidon_sign(sk, m, rho, pp, jj) + (m,) for sk, m, rho in keys]
    rows = list(valid)
    corrupt = [lambda v, o: ((v[0] + 1) % FS, v[1], v[2], v[3]), lambda v, o: (0, v[1], v[2], v[3]), lambda v, o: (v[0], v[1], v[2], (v[3] + 1) % R),
               lambda v, o: (v[0], o[1], v[2], v[3]), lambda v, o: (v[0], v[1], o[2], v[3]), lambda v, o: (v[0], (R - v[1]) % R, v[2], v[3]),
               lambda v, o: (v[0], rootless, v[2], v[3]), lambda v, o: (v[0], v[1], outside, v[3])]
    for j in range(72):
        rows.append(corrupt[j % 8](valid[j % 48], valid[(j + 7) % 48]))
    want = [fc.eddsaposeidon_verify(s, r, a, m, pp, jj) for s, r, a, m in rows]
    assert all(want[:48])
    m_is_r = [False] * len(rows)
    for j in range(5):                       # s + Fs: the oracle would accept, the ABI rejects
        v = valid[5 + j]
        assert fc.eddsaposeidon_verify(v[0] + FS, v[1], v[2], v[3], pp, jj) and v[0] + FS < 1 << 256
        rows.append((v[0] + FS, v[1], v[2], v[3])); want.append(False); m_is_r.append(False)
    for j in range(4):                       # m = the limbs of r
        v = valid[10 + j]
        rows.append((v[0], v[1], v[2], 0)); want.append(False); m_is_r.append(True)
    order = list(range(1, len(rows)))
    rnd.shuffle(order)
    order = [0] + order
    rows, want, m_is_r = [rows[i] for i in order], [want[i] for i in order], [m_is_r[i] for i in order]
    assert len(rows) == 129 and 3 * sum(want) >= 129 and 3 * (129 - sum(want)) >= 129
    return tuple(rows), tuple(want), tuple(m_is_r)


def verify_arrays(n):
    """s as ints; r, a, m as Montgomery limb arrays (m carries the out-of-range rows)"""
    from fawkes_crypto_amd import api
    rows, want, m_is_r = verify_cases()
    s = [row[0] for row in rows[:n]]
    r, a, m = (api._fr_rows([row[k] for row in rows[:n]]) for k in (1, 2, 3))
    for i in range(n):
        if m_is_r[i]:
            m[i] = api.int_to_limbs(R)
    return s, r, a, m, list(want[:n])


def test_verify_matches_oracle(ctx):
    dp = device_params()
    for n in SIZES:
        s, r, a, m, want = verify_arrays(n)
        assert ctx.eddsa_verify(dp, s, r, a, m) == want, n
    assert ctx.eddsa_verify(dp, [], [], [], []) == []


def test_verify_dev_matches_oracle(ctx):
    from fawkes_crypto_amd import api
    dp = device_params()
    for n in SIZES:
        s, r, a, m, want = verify_arrays(n)
        bufs = [ctx.dev_alloc(32 * n) for _ in range(4)] + [ctx.dev_alloc(n)]
        try:
            for d, arr in zip(bufs, (api._u256_rows(s), r, a, m)):
                ctx.upload(d, arr)
            ctx.eddsa_verify_dev(dp, bufs[0], bufs[1], bufs[2], bufs[3], n, bufs[4])
            ctx.sync()
            assert [bool(v) for v in ctx.download(bufs[4], n, np.uint8)] == want, n
        finally:
            for d in bufs:
                ctx.dev_free(d)


# ---------------------------------------------------------------------------------------------- sign
@functools.lru_cache(maxsize=None)
def sign_cases():
    jj, pp, rnd = curve(), oracle_params(), random.Random(2718)
    keys = [(1, rnd.randrange(R), rnd.randrange(FS)), (0, rnd.randrange(R), rnd.randrange(FS)), (rnd.randrange(FS), rnd.randrange(R), 0),
            (rnd.randrange(FS), 0, rnd.randrange(FS)), (rnd.randrange(FS), R - 1, rnd.randrange(FS)), (FS - 1, rnd.randrange(R), FS - 1)]
    keys += [(rnd.randrange(FS), rnd.randrange(R), rnd.randrange(FS)) for _ in range(65)]
    return tuple(keys), tuple(fc.eddsaposeidon_sign(sk, m, rho, pp, jj) for sk, m, rho in keys)


def test_sign_matches_oracle_and_verifies(ctx):
    dp = device_params()
    keys, want = sign_cases()
    for n in (1, 63, 64, 65, len(keys)):
        s, r_x, a_x = ctx.eddsa_sign(dp, [k[0] for k in keys[:n]], [k[1] for k in keys[:n]], [k[2] for k in keys[:n]])
        assert list(zip(s, r_x, a_x)) == list(want[:n]), n
    assert all(ctx.eddsa_verify(dp, s, r_x, a_x, [k[1] for k in keys]))
    assert ctx.eddsa_sign(dp, [], [], []) == ([], [], [])


def test_sign_with_the_library_nonce(ctx):
    """rhos=None: the nonce is Blake2s-256("__fawkes"; sk | m) mod Fs, computed here with hashlib"""
    jj, pp, dp = curve(), oracle_params(), device_params()
    keys, _ = sign_cases()
    sks, ms = [k[0] for k in keys[:16]], [k[1] for k in keys[:16]]
    rhos = [int.from_bytes(hashlib.blake2s(sk.to_bytes(32, 'little') + m.to_bytes(32, 'little'), digest_size=32, person=b'__fawkes').digest(), 'little') % FS
            for sk, m in zip(sks, ms)]
    want = [fc.eddsaposeidon_sign(sk, m, rho, pp, jj) for sk, m, rho in zip(sks, ms, rhos)]
    s, r_x, a_x = ctx.eddsa_sign(dp, sks, ms)
    assert list(zip(s, r_x, a_x)) == want
    assert all(ctx.eddsa_verify(dp, s, r_x, a_x, ms))


def test_sign_reproduces_the_golden_vector(ctx):
    g = json.load(open(GOLDEN))
    s, r_x, a_x = ctx.eddsa_sign(device_params(), [int(g['sk'], 16)], [int(g['m'], 16)], [int(g['rho'], 16)])
    assert ['%064x' % v[0] for v in (s, r_x, a_x)] == [g['signature']['s'], g['signature']['r_x'], g['signature']['a_x']]


# ---------------------------------------------------------------------------------------------- arguments
def test_argument_checks(ctx):
    import fawkes_crypto_amd as fk
    dp, t3 = device_params(), fk.PoseidonParams(3, 8, 53)
    for call in (lambda: ctx.eddsa_verify(t3, [1], [0], [0], [0]), lambda: ctx.eddsa_sign(t3, [1], [2], [3]), lambda: ctx.eddsa_sign(dp, [FS], [2], [3]),
                 lambda: ctx.eddsa_sign(dp, [1], [2], [FS])):
        with pytest.raises(fk.FkError) as e:
            call()
        assert e.value.code == 1
    assert ctx.eddsa_verify(dp, [], [], [], []) == [] and ctx.jubjub_mul(None, []) == [] and ctx.jubjub_decompress([]) == []
    assert ctx.eddsa_verify(dp, [1], [0], [0], [0]) == [False]             # the context is still usable after a refused call
