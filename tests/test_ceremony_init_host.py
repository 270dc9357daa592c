"""The initial key's host references (include/fawkes_hip_ceremony_init.h through fawkes_crypto_amd/ceremony_init.py; no GPU): the header
against the library and the ctypes table, the transforms over group elements against the oracle's scalar transform mapped through its
g1_mul / g2_mul, the key from a transcript against THE ORACLE'S OWN SETUP WITH gamma = delta = 1, the transcript check's sums against
Python integers and its verdicts against the Python pairing, every tamper with exactly its flags cleared, and the argument errors.
Every comparison is exact."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import c_oracle as co
import ceremony_init_cases as ic
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import ceremony_init as CI
from helpers import rand_fr_mont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
HEADER = os.path.join(INCLUDE, 'fawkes_hip_ceremony_init.h')


@pytest.fixture(scope='module', autouse=True)
def _oracle(oracle):
    return oracle


# ---------------------------------------------------------------- the header, the library, the ctypes table
def _declared():
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b(fk_\w+)\s*\(([^()]*)\)\s*;', text):
        out[name] = len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])
    return out


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(CI.PROTOTYPES) and len(decl) == 8
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(CI.PROTOTYPES[name][1]) == nargs, name
    # no name collides with the pinned ABI or with another extra table
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    others = [fk.ceremony.PROTOTYPES, fk.witness.PROTOTYPES, fk.verify_agg.PROTOTYPES, fk.check.PROTOTYPES, fk.merkle.PROTOTYPES, fk.sparse_merkle.PROTOTYPES,
              fk.merkle_set.PROTOTYPES, fk.batch.PROTOTYPES, fk.batch.CHECK_PROTOTYPES]
    for table in others:
        assert not set(decl) & set(table)
    for name in ('PowersOfTau', 'PowersReport', 'g1_ntt', 'g2_ntt', 'initial_key', 'initial_key_host', 'initial_image', 'check_powers', 'check_powers_host'):
        assert getattr(fk, name) is getattr(CI, name), name


def test_header_compiles_alone_as_c99():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include "fawkes_hip_ceremony_init.h"\nint main(void) { fk_powers_desc d; fk_powers_report r; d.n_tau_g1 = 3; r.accept = 0; '
                             'return (int)d.n_tau_g1 - 3 + r.accept; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', INCLUDE, src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])


# ---------------------------------------------------------------- transforms over group elements
@pytest.mark.parametrize('log_n', range(7))
def test_transforms_are_the_oracles_scalar_transform_in_the_exponent(log_n):
    n = 1 << log_n
    s = rand_fr_mont(np.random.default_rng(100 + log_n), n)
    for mul, ntt, gen in ((co.g1_mul, CI.g1_ntt, ic.G1), (co.g2_mul, CI.g2_ntt, ic.G2)):
        pts = np.array([mul(gen, s[i]) for i in range(n)])
        fwd = ntt(None, pts)
        assert fwd.tobytes() == np.array([mul(gen, x) for x in co.fr_ntt(s)]).tobytes()
        assert ntt(None, pts, inverse=True).tobytes() == np.array([mul(gen, x) for x in co.fr_ntt(s, inverse=True)]).tobytes()
        assert ntt(None, fwd, inverse=True).tobytes() == pts.tobytes()


# ---------------------------------------------------------------- the initial key
@pytest.mark.parametrize('shape', ['one', 'tiny', 'small', 'unused'])
def test_key_from_powers_is_the_oracles_setup(shape):
    c = ic.case(shape)
    p = fk.initial_key_host(ic.transcript(), c.r1cs)             # (the transcript is longer than any of these shapes needs)
    assert (p.m, p.num_input, p.num_aux) == (c.m, c.cs.num_input, c.cs.num_aux) and p.key is None
    ic.assert_key(dict(h=p.h, l=p.l, a=p.a, b_g1=p.b_g1, b_g2=p.b_g2), p.vk_full, p.ic, c.key)
    assert p.vk_full['delta_g1'].tobytes() == ic.G1.tobytes() and p.vk_full['gamma_g2'].tobytes() == p.vk_full['delta_g2'].tobytes() == ic.G2.tobytes()
    if shape == 'unused':
        # the variable in no constraint: infinity in l, skipped by a and b; the one in B only: in b, not in a
        assert not p.l[-1].any() and p.l[-2].any()
        nv = c.cs.num_input + c.cs.num_aux
        base = ic.case('small').key
        assert p.a.shape[0] == np.array(base.a).shape[0] <= nv - 2 and p.b_g1.shape[0] == np.array(base.b_g1).shape[0] + 1
    # exactly the prefix is enough
    q = fk.initial_key_host(ic.transcript().prefix(c.m), c.r1cs)
    assert q.h.tobytes() == p.h.tobytes() and q.l.tobytes() == p.l.tobytes()


# ---------------------------------------------------------------- the transcript check
def test_check_accepts_the_honest_transcript():
    pw = ic.transcript()
    for m in (2, 4, 64):
        rep = fk.check_powers_host(pw, m, ic.SEED)
        assert rep.flags() == ic.expect_flags() and rep.accept is True and rep.seed == ic.SEED
    rep = fk.check_powers_host(pw, 4, ic.SEED)                   # 'tiny': the sums over Python integers, the verdicts by the Python pairing
    assert rep.sums() == ic.sums_py(pw, 4, ic.SEED)
    assert ic.verdicts_py(pw, rep) == {n: True for n in ic.FLAGS if n != 'gen_ok'}
    rep2 = fk.check_powers_host(pw, 4, ic.OTHER_SEED)            # the weights depend on the seed, the verdict does not
    assert rep2.accept is True and rep2.s_tau_g1 != rep.s_tau_g1


@pytest.mark.parametrize('kind', ic.TAMPERS)
def test_check_rejects_with_exactly_the_expected_flags(kind):
    bad = ic.tamper(ic.transcript(), 64, kind)
    rep = fk.check_powers_host(bad, 64, ic.SEED)
    assert rep.flags() == ic.expect_flags(kind), kind
    assert rep.accept is False


@pytest.mark.parametrize('kind', ['tau_g1_mid', 'tau_g2_1_other', 'beta_g2_other'])
def test_verdicts_are_the_python_pairings(kind):
    bad = ic.tamper(ic.transcript(), 4, kind)
    rep = fk.check_powers_host(bad, 4, ic.SEED)
    assert rep.sums() == ic.sums_py(bad, 4, ic.SEED)
    want = ic.verdicts_py(bad, rep)
    assert {n: getattr(rep, n) for n in want} == want
    assert want == {n: v for n, v in ic.expect_flags(kind).items() if n in want}


# ---------------------------------------------------------------- argument errors
def _refused(fn, code=1, word=None):
    with pytest.raises(fk.FkError) as e:
        fn()
    assert e.value.code == code
    if word:
        assert word in str(e.value), str(e.value)


def test_argument_errors():
    pw, c = ic.transcript(), ic.case('tiny')
    m = c.m
    short = dict(tau_g1=pw.tau_g1[:2 * m - 2], tau_g2=pw.tau_g2[:m - 1], alpha_tau_g1=pw.alpha_tau_g1[:m - 1], beta_tau_g1=pw.beta_tau_g1[:m - 1])
    for name, arr in short.items():                            # a transcript that is too short, once per array: the message names it
        bad = pw.prefix(m).replace(**{name: arr})
        _refused(lambda: fk.initial_key_host(bad, c.r1cs), 1, name + ' ')
        _refused(lambda: fk.check_powers_host(bad, m, ic.SEED), 1, name + ' ')
    lib = CI._lib()
    d, rep = pw.desc(), CI.PowersReportStruct()
    seed = np.frombuffer(ic.SEED, np.uint8)
    assert lib.fk_powers_check_host(None, 4, seed.ctypes.data, rep) == 1                     # null pointers
    assert lib.fk_powers_check_host(d, 4, None, rep) == 1
    assert lib.fk_powers_check_host(d, 4, seed.ctypes.data, None) == 1
    assert lib.fk_powers_check_host(d, 1, seed.ctypes.data, rep) == 1
    null_array = pw.desc()
    null_array.beta_g2 = None
    assert lib.fk_powers_check_host(null_array, 4, seed.ctypes.data, rep) == 1
    out = np.zeros(6 * 128, np.uint8)
    assert lib.fk_key_from_powers_host(d, None, None, None, None, None, None, None, out.ctypes.data, None) == 1
    assert lib.fk_g1_ntt(None, None, 2, 0, None) == 1 and lib.fk_g2_ntt(None, None, 2, 1, None) == 1
    assert lib.fk_g1_ntt(None, out.ctypes.data, 28, 0, out.ctypes.data) == 2                  # FK_ERR_DOMAIN_TOO_LARGE
    with pytest.raises(ValueError):
        fk.g1_ntt(None, np.zeros((3, 64), np.uint8))
    with pytest.raises(ValueError):
        fk.check_powers_host(pw, 4, b'short')
    A, B, Cm = c.r1cs.mats
    no_input = fk.R1cs(0, c.r1cs.num_aux, A, B, Cm)                                           # num_input == 0
    _refused(lambda: fk.initial_key_host(pw, no_input), 1, 'num_input')
    col = A[1].copy()
    col[0] = c.r1cs.num_input + c.r1cs.num_aux                                                 # a column index out of range
    _refused(lambda: fk.initial_key_host(pw, fk.R1cs(c.r1cs.num_input, c.r1cs.num_aux, (A[0], col, A[2]), B, Cm)), 1, 'out of range')
