"""Phase 1 of the key ceremony, the host references (include/fawkes_hip_powers.h through fawkes_crypto_amd/powers.py; no GPU): the header
against the library and the ctypes table, a point times its own power against the oracle's g1_mul / g2_mul of scalars computed in Python,
a contribution (and a chain of two) against transcripts MADE BY THE ORACLE, the classes of sample points, the update check's flags for
the honest update and every tamper with exactly its flags cleared, the step verdicts against the Python pairing, and the refusals.
Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import c_oracle as co
import ceremony_cases as cc
import ceremony_init_cases as ic
import fawkes_crypto_amd as fk
import powers_cases as pc
from fawkes_crypto_amd import powers as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
HEADER = os.path.join(INCLUDE, 'fawkes_hip_powers.h')
R = pc.R
M = 8


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
    assert sorted(decl) == sorted(PW.PROTOTYPES) and len(decl) == 11
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(PW.PROTOTYPES[name][1]) == nargs, name
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    for table in (fk.ceremony.PROTOTYPES, fk.ceremony_init.PROTOTYPES, fk.witness.PROTOTYPES, fk.verify_agg.PROTOTYPES, fk.check.PROTOTYPES, fk.merkle.PROTOTYPES,
                  fk.sparse_merkle.PROTOTYPES, fk.merkle_set.PROTOTYPES, fk.batch.PROTOTYPES, fk.batch.CHECK_PROTOTYPES):
        assert not set(decl) & set(table)
    for name in ('PowersPublic', 'PointsReport', 'PowersUpdateReport', 'new_powers', 'contribute', 'contribute_host', 'scale_powers', 'scale_powers_dev',
                 'validate_points', 'check_update', 'check_update_host'):
        assert getattr(fk, name) is getattr(PW, name), name


def test_header_compiles_alone_as_c99_and_the_structs_have_the_mirrors_sizes():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include <stdio.h>\n#include "fawkes_hip_powers.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(fk_powers_out), '
                             'sizeof(fk_powers_public), sizeof(fk_points_report), sizeof(fk_powers_update_report)); return 0; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', INCLUDE, src, '-o', os.path.join(td, 'alone')])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(td, 'alone')]).split()]
    assert sizes == [C.sizeof(PW.PowersOutStruct), C.sizeof(PW.PowersPublicStruct), C.sizeof(PW.PointsReportStruct), C.sizeof(PW.PowersUpdateReportStruct)]


# ---------------------------------------------------------------- a point times its own power
@pytest.mark.parametrize('group', ['g1', 'g2'])
@pytest.mark.parametrize('first', [0, 5, (1 << 32) + 5])
def test_scale_is_the_oracles_multiplication_by_the_python_scalar(group, first):
    mul, base = (co.g1_mul, pc.before(M).tau_g1) if group == 'g1' else (co.g2_mul, pc.before(M).tau_g2)
    pts = base[:5].copy()
    pts[3] = 0                                                             # the point at infinity stays
    for x, c in ((pc.X, 1), (2, pc.Y), (R - 1, pc.Z)):
        got = fk.scale_powers(None, pts, pc.mont(x), None if c == 1 else pc.mont(c), first=first)
        want = np.array([mul(pts[i], pc.mont(c * pow(x, first + i, R))) for i in range(5)])
        assert got.tobytes() == want.tobytes() and not got[3].any()
    assert fk.scale_powers(None, pts[:0], pc.mont(3)).shape == pts[:0].shape


# ---------------------------------------------------------------- contribute
def test_new_powers_is_the_generators():
    pw = fk.new_powers(M)
    assert pw.tau_g1.shape == (2 * M - 1, 64) and pw.tau_g2.shape == (M, 128) and pw.alpha_tau_g1.shape == (M, 64) and pw.beta_tau_g1.shape == (M, 64)
    assert all(row.tobytes() == ic.G1.tobytes() for arr in (pw.tau_g1, pw.alpha_tau_g1, pw.beta_tau_g1) for row in arr)
    assert all(row.tobytes() == ic.G2.tobytes() for row in pw.tau_g2) and pw.beta_g2.tobytes() == ic.G2.tobytes()


def test_contribution_to_the_generators_is_the_oracles_transcript():
    got, pub = fk.contribute_host(fk.new_powers(M), pc.mont(pc.TAU), pc.mont(pc.ALPHA), pc.mont(pc.BETA))
    pc.same_transcript(got, pc.before(M))
    assert (pub.x_g2.tobytes(), pub.y_g2.tobytes(), pub.z_g2.tobytes()) == (pc.g2(pc.TAU).tobytes(), pc.g2(pc.ALPHA).tobytes(), pc.g2(pc.BETA).tobytes())


def test_chained_contribution_is_the_oracles_transcript_of_the_products():
    src = pc.before(M)
    keep = {n: getattr(src, n).copy() for n in PW.ARRAYS}
    got, pub = fk.contribute_host(src, pc.mont(pc.X), pc.mont(pc.Y), pc.mont(pc.Z))
    pc.same_transcript(got, pc.after(M))
    want = pc.public()
    assert (pub.x_g2.tobytes(), pub.y_g2.tobytes(), pub.z_g2.tobytes()) == (want.x_g2.tobytes(), want.y_g2.tobytes(), want.z_g2.tobytes())
    assert all(getattr(src, n).tobytes() == keep[n].tobytes() for n in PW.ARRAYS)          # the input is only read


# ---------------------------------------------------------------- validate points
@pytest.mark.parametrize('group', ['g1', 'g2'])
def test_validate_sorts_one_point_of_every_class(group):
    classes = ('good',) + pc.CLASSES[group] + ('good',)
    pts = np.array([pc.bad_point(group, c, salt=i) for i, c in enumerate(classes)])
    rep = fk.validate_points(None, pts)
    assert rep.counts() == {c: int(c in classes) for c in ('infinity', 'range', 'curve', 'subgroup')} and rep.first_bad == 1 and not rep.ok
    for i, c in enumerate(classes):                                        # one at a time: exactly its class
        one = fk.validate_points(None, pts[i:i + 1])
        assert one.counts() == {k: int(k == c) for k in ('infinity', 'range', 'curve', 'subgroup')}
        assert one.first_bad == (None if c == 'good' else 0) and one.ok is (c == 'good')
    good = pc.before(M).tau_g1 if group == 'g1' else pc.before(M).tau_g2
    rep = fk.validate_points(None, good)
    assert rep.ok and rep.first_bad is None
    assert fk.validate_points(None, good[:0]).ok


# ---------------------------------------------------------------- check an update
def test_update_check_accepts_the_honest_update():
    for m in (2, 4, M):
        b, a, p = pc.tampered(m, None)
        rep = fk.check_update_host(b, a, p, m, pc.SEED)
        pc.assert_update_report(rep, m, None)
        assert rep.after.seed == pc.SEED
    b, a, p = pc.tampered(4, None)
    rep = fk.check_update_host(b, a, p, 4, pc.SEED)
    # the embedded report: the sums over Python integers, the verdicts by the Python pairing; the steps by the Python pairing
    assert rep.after.sums() == ic.sums_py(a, 4, pc.SEED)
    assert ic.verdicts_py(a, rep.after) == {n: True for n in ic.FLAGS if n != 'gen_ok'}
    assert cc.pairing_eq_py(a.tau_g1[1], ic.G2, b.tau_g1[1], p.x_g2) and cc.pairing_eq_py(a.alpha_tau_g1[0], ic.G2, b.alpha_tau_g1[0], p.y_g2)
    assert cc.pairing_eq_py(a.beta_tau_g1[0], ic.G2, b.beta_tau_g1[0], p.z_g2)
    same = fk.check_update_host(a, a, fk.PowersPublic(ic.G2, ic.G2, ic.G2), 4, pc.SEED)          # x = y = z = 1 is a valid contribution
    assert same.accept is True and same.changed is False


@pytest.mark.parametrize('kind', pc.TAMPERS)
def test_update_check_rejects_with_exactly_the_expected_flags(kind):
    b, a, p = pc.tampered(M, kind)
    pc.assert_update_report(fk.check_update_host(b, a, p, M, pc.SEED), M, kind)


def test_step_verdicts_are_the_python_pairings_for_a_wrong_public_part():
    b, a, p = pc.tampered(4, 'pub_y')
    rep = fk.check_update_host(b, a, p, 4, pc.SEED)
    want = dict(step_tau=cc.pairing_eq_py(a.tau_g1[1], ic.G2, b.tau_g1[1], p.x_g2), step_alpha=cc.pairing_eq_py(a.alpha_tau_g1[0], ic.G2, b.alpha_tau_g1[0], p.y_g2),
                step_beta=cc.pairing_eq_py(a.beta_tau_g1[0], ic.G2, b.beta_tau_g1[0], p.z_g2))
    assert {n: getattr(rep, n) for n in want} == want == dict(step_tau=True, step_alpha=False, step_beta=True)


def test_a_single_point_off_the_curve_is_never_paired():
    b, a, p = pc.tampered(4, None)
    t = a.tau_g1.copy()
    t[1] = pc.bad_point('g1', 'curve')
    rep = fk.check_update_host(b, a.replace(tau_g1=t), p, 4, pc.SEED)
    assert rep.points['tau_g1'].counts()['curve'] == 1 and rep.points['tau_g1'].first_bad == 1
    assert rep.flags() == dict(pc.expect_own(), points_ok=False, step_tau=False)
    assert rep.after.flags() == dict(pc.expect_after(), tau_pair=False, ratio_tau_g1=False, ratio_tau_g2=False)
    assert not any(rep.after.s_tau_g1) and not any(rep.after.s_tau_g1_next) and any(rep.after.s_alpha)
    bad_pub = p.replace(z_g2=pc.bad_point('g2', 'range'))
    rep = fk.check_update_host(b, a, bad_pub, 4, pc.SEED)
    assert rep.flags() == dict(pc.expect_own(), step_beta=False) and rep.after.accept is True


# ---------------------------------------------------------------- refusals
def _refused(fn, code=1, word=None):
    with pytest.raises(fk.FkError) as e:
        fn()
    assert e.value.code == code
    if word:
        assert word in str(e.value), str(e.value)


def test_refusals():
    b, a, p = pc.tampered(4, None)
    ok = pc.mont(5)
    zero, big = np.zeros(4, np.uint64), np.full(4, 0xffffffffffffffff, np.uint64)
    r_limbs = np.frombuffer(R.to_bytes(32, 'little'), np.uint64)
    for bad in (zero, big, r_limbs):                                      # a secret that is zero or not below r, in every position
        for args in ((bad, ok, ok), (ok, bad, ok), (ok, ok, bad)):
            _refused(lambda: fk.contribute_host(b, *args), 1, 'nonzero')
        _refused(lambda: fk.scale_powers(None, b.tau_g1, bad), 1, 'nonzero')
        _refused(lambda: fk.scale_powers(None, b.tau_g1, ok, bad), 1, 'nonzero')
    _refused(lambda: fk.scale_powers(None, b.tau_g1, ok, first=(1 << 64) - 3), 1, '2^64')
    _refused(lambda: fk.contribute_host(b.replace(tau_g1=b.tau_g1[:1]), ok, ok, ok), 1, 'too short')          # nothing an update check could bind
    _refused(lambda: fk.contribute_host(b.replace(alpha_tau_g1=b.alpha_tau_g1[:0]), ok, ok, ok), 1, 'too short')
    # a transcript too short for m is a verdict, not an error: shape_ok = 0 and nothing else looked at
    for bb, aa in ((b.replace(tau_g1=b.tau_g1[:6]), a), (b, a.replace(beta_tau_g1=a.beta_tau_g1[:3]))):
        rep = fk.check_update_host(bb, aa, p, 4, pc.SEED)
        assert rep.flags() == {n: False for n in PW.FLAGS} and rep.accept is False and rep.after.accept is False
        assert all(r.ok and r.first_bad is None for r in rep.points.values())
    _refused(lambda: fk.check_update_host(b, a, p, 1, pc.SEED), 1, 'at least 2')
    with pytest.raises(ValueError):
        fk.check_update_host(b, a, p, 4, None)
    with pytest.raises(ValueError):
        fk.validate_points(None, np.zeros((3, 65), np.uint8))
    with pytest.raises(ValueError):
        fk.new_powers(0)
    # null pointers
    lib = PW._lib()
    db, da, ps, st = b.desc(), a.desc(), p.struct(), PW.PowersUpdateReportStruct()
    seed = np.frombuffer(pc.SEED, np.uint8)
    assert lib.fk_powers_update_check_host(None, da, ps, 4, seed.ctypes.data, st) == 1
    assert lib.fk_powers_update_check_host(db, None, ps, 4, seed.ctypes.data, st) == 1
    assert lib.fk_powers_update_check_host(db, da, None, 4, seed.ctypes.data, st) == 1
    assert lib.fk_powers_update_check_host(db, da, ps, 4, None, st) == 1
    assert lib.fk_powers_update_check_host(db, da, ps, 4, seed.ctypes.data, None) == 1
    null_array = a.desc()
    null_array.tau_g2 = None
    assert lib.fk_powers_update_check_host(db, null_array, ps, 4, seed.ctypes.data, st) == 1
    out, pub = PW.PowersOutStruct(), PW.PowersPublicStruct()
    assert lib.fk_powers_contribute_host(db, ok.ctypes.data, ok.ctypes.data, ok.ctypes.data, out, pub) == 1          # an output without arrays
    assert lib.fk_powers_contribute_host(None, ok.ctypes.data, ok.ctypes.data, ok.ctypes.data, out, pub) == 1
    assert lib.fk_powers_contribute_host(db, None, ok.ctypes.data, ok.ctypes.data, out, pub) == 1
    assert lib.fk_powers_new(4, None) == 1 and lib.fk_powers_new(4, out) == 1
    rep = PW.PointsReportStruct()
    assert lib.fk_points_validate(None, None, 3, 0, rep) == 1 and lib.fk_points_validate(None, b.tau_g1.ctypes.data, 3, 0, None) == 1
    assert lib.fk_points_validate(None, b.tau_g1.ctypes.data, 3, 2, rep) == 1
    assert lib.fk_g1_scale_powers(None, None, 3, 0, ok.ctypes.data, ok.ctypes.data, None) == 1
    assert lib.fk_g2_scale_powers(None, b.tau_g2.ctypes.data, 3, 0, None, ok.ctypes.data, b.tau_g2.ctypes.data) == 1
