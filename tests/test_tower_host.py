"""The pairing tower of csrc/pairing.hpp by VALUE, on the host: Fq6T, Fq12T, miller_loop, miller_loop_proj and final_exponentiation
instantiated with Fq (the type fk_verify uses), each called by a thin wrapper of the test-only library (csrc/fieldtest_tower.hip,
where = host: no HIP call, no GPU) and compared with the polynomial-basis reference of _tower_ref.py.

Every other test of pairing.hpp asserts a verdict, and every wrong case the suite has differs from one in all twelve coefficients:
an is_one() that forgot a coefficient, a pow that mishandles a leading zero word, an inv wrong on an element with a zero half or a
wrong sparse product would pass them all.  The cases and checks are those of test_gpu_tower_ops.py (_tower_cases.py); here they also
prove the case lists and the reference on a machine without a GPU.
"""
import random

import pytest

import bn254_ref as ref
import _tower_cases as tc
import _tower_ref as tr
from _fieldtest import MONT_R, TOWER_OPS, TYPE, FieldTestLib

LIB = FieldTestLib()
WHERE = 'host'


@pytest.fixture(scope='module')
def pairings():
    return tc.Pairings(LIB, WHERE)


def test_library_offers_the_tower_operations():
    """the library's table and the tests' agree exactly, shapes included"""
    words = {12: 96, 6: 48, 2: 16}
    for i, op in enumerate(TOWER_OPS):
        shape = LIB.tower_shape(i)
        if op in tc.ARITH:
            n_out = {'f6_mul_xi': 2}.get(op, 6 if op.startswith('f6') else 12)
            assert shape == (sum(words[k] for k in tc.ARITH[op][0]), words[n_out]), op
    assert LIB.tower_shape(TOWER_OPS.index('f12_is_one')) == (96, 1)
    assert LIB.tower_shape(TOWER_OPS.index('f12_pow')) == (96 + 24 + 1, 96)
    assert LIB.tower_shape(TOWER_OPS.index('miller_loop')) == LIB.tower_shape(TOWER_OPS.index('miller_loop_proj')) == (48, 96)
    assert LIB.tower_shape(TOWER_OPS.index('final_exp')) == (96, 96)
    assert LIB.tower_shape(len(TOWER_OPS)) is None and LIB.tower_shape(-1) is None
    assert set(tc.ARITH) | {'f12_is_one', 'f12_pow', 'miller_loop', 'miller_loop_proj', 'final_exp'} == set(TOWER_OPS)


def test_basis_map_is_a_ring_isomorphism_on_the_generators():
    """the one tower-aware piece of the reference: u^2 = -1, v^3 = xi, w^2 = v hold in the polynomial basis, and the map inverts"""
    e = lambda t, val=1: tr.to_poly(tc.unit(12, t, val))
    u, v, w, one = e(1), e(2), e(6), e(0)
    assert one == tr.ONE
    assert ref.f12_mul(u, u) == [tr.P - 1] + [0] * 11
    assert ref.f12_mul(w, w) == v
    assert ref.f12_mul(v, ref.f12_mul(v, v)) == tr.to_poly([9, 1] + [0] * 10)
    rnd = random.Random(5)
    for _ in range(20):
        a = [rnd.randrange(tr.P) for _ in range(12)]
        assert tr.from_poly(tr.to_poly(a)) == a


def test_conjugation_is_the_power_p6():
    rnd = random.Random(6)
    for _ in range(2):
        a = [rnd.randrange(tr.P) for _ in range(12)]
        assert tr.to_poly(tc.ARITH['f12_conj'][1](a)) == ref.f12_pow(tr.to_poly(a), tr.P ** 6)


def test_final_exponentiation_constants():
    """the two exponents the product raises to, and the factorisation final_exponentiation rests on"""
    p, r = tr.P, tr.R_ORDER
    p2p1, hard = tc.fexp_constants()
    assert p2p1 == p * p + 1
    assert (p ** 4 - p * p + 1) % r == 0 and hard == (p ** 4 - p * p + 1) // r
    assert (p ** 6 - 1) * (p * p + 1) * ((p ** 4 - p * p + 1) // r) == (p ** 12 - 1) // r == tr.FINAL_EXPONENT
    assert (p ** 12 - 1) % r == 0
    assert tr.FINAL_EXPONENT % (p ** 6 - 1) == 0 and (p ** 6 - 1) % (p * p - 1) == 0       # every proper subfield goes to one


@pytest.mark.parametrize('op', tc.ARITH_OPS)
def test_tower_arithmetic(op):
    tc.check_arith(LIB, WHERE, op)


def test_is_one_is_true_on_exactly_one():
    tc.check_is_one(LIB, WHERE)


def test_pow():
    tc.check_pow(LIB, WHERE)


def test_final_exponentiation():
    tc.check_final_exp(LIB, WHERE)


def test_miller_loop_value(pairings):
    tc.check_miller_value(pairings)


def test_miller_loop_proj_differs_by_a_factor_in_fq2(pairings):
    tc.check_proj_ratio(pairings)


def test_pairing_value_and_bilinearity(pairings):
    tc.check_pairing_value(pairings)


def test_wrong_shapes_are_refused_with_a_code():
    """the error contract of ft_run: a code and a message, never an abort"""
    import ctypes as C
    lib = LIB.lib()
    out = C.create_string_buffer(96 * 4)
    assert lib.ft_tower_run(0, 1, b'\0' * 384, 95, out, 48, 1) == 1 and b'words' in lib.ft_last_error()
    assert lib.ft_tower_run(99, 1, b'\0' * 384, 96, out, 48, 1) == 1
    assert lib.ft_tower_run(0, 2, b'\0' * 384, 96, out, 48, 1) == 1
    assert lib.ft_tower_run(0, 1, b'\0' * 384, 96, out, 48, 0) == 1
    assert lib.ft_tower_run(0, 1, None, 96, out, 48, 1) == 1


# ------------------------------------------------------------------------------------------------ the new field and point cases
def test_new_field_references_are_consistent():
    """the references test_gpu_field_ops.py adds for inv, pow, pow_u64 and from_u64, held against each other without the library:
    a * inv(a) is the Montgomery one, pow(a, p - 2) is inv(a), pow_u64 and pow agree on a 64-bit exponent"""
    import test_gpu_field_ops as fo
    for name in ('Fq', 'FqL', 'Fr', 'Fq2', 'Fq2L'):
        t = TYPE[name]
        one = (MONT_R, 0) if t.fq2 else MONT_R
        for c in fo.targeted(t, 'inv')[:40]:
            a = tuple(zip(c[0::2], c[1::2]))[0] if t.fq2 else c[0]
            (ai,) = fo.REF['inv'][3](t, (a,))
            prod = fo.mul(t, a, ai)
            zero = fo.is_zero(t, a)
            assert fo.check_element(t, tuple(v % t.p for v in prod) if t.fq2 else prod % t.p, (0, 0) if zero and t.fq2 else 0 if zero else one, exact=True) is None
            if not t.fq2:
                assert (fo.REF['pow'][3](t, (a, t.p - 2))[0] - ai) % t.p == 0
                assert (fo.REF['pow_u64'][3](t, (a, (7 << 64) | 12345))[0] - fo.REF['pow'][3](t, (a, 12345))[0]) % t.p == 0
        if not t.fq2:
            assert fo.REF['from_u64'][3](t, ((5 << 64) | 9,))[0] % t.p == 9 * MONT_R % t.p
