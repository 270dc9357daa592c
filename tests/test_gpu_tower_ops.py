"""The pairing tower of csrc/pairing.hpp by VALUE, on the device: Fq6T, Fq12T, miller_loop, miller_loop_proj and final_exponentiation
instantiated with FqC (the only type the device pairing code uses), one lane per case in 64-thread blocks as verify_batch_kernel and
agg_miller_kernel run them, each called by a thin wrapper of the test-only library (csrc/fieldtest_tower.hip) and compared with the
polynomial-basis reference of _tower_ref.py, which has no tower, no Karatsuba and no sparse product.

The cases and checks are those of test_tower_host.py (_tower_cases.py), which runs them through the host instantiation; the
expected values are computed once per process.  Contract: every result limb image equals the exact value mod p, bit for bit.

Known limit, as in test_gpu_field_ops.py: the wrappers are separate kernels; the scheduling around the same text in
verify_batch_kernel is the compiler's, and the verdict tests remain the check on that.
"""
import pytest

import _tower_cases as tc
from _fieldtest import FieldTestLib

pytestmark = pytest.mark.gpu

LIB = FieldTestLib()        # the module-level guard: after one failed call nothing more is launched from this module
WHERE = 'device'


@pytest.fixture(scope='module')
def pairings():
    return tc.Pairings(LIB, WHERE)


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
    """66 lanes: lanes with a point at infinity return early beside lanes that run the loop"""
    tc.check_miller_value(pairings)


def test_miller_loop_proj_differs_by_a_factor_in_fq2(pairings):
    tc.check_proj_ratio(pairings)


def test_pairing_value_and_bilinearity(pairings):
    tc.check_pairing_value(pairings)
