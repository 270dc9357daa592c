"""The R1CS check on the device (csrc/check.hip through fawkes_crypto_amd/check.py) against the host reference fk_r1cs_check on the same
inputs -- the whole report, the bitmap, the group flags -- and, since it costs nothing, against the oracle's own expectation
(tests/check_cases.py): explicit systems around the wave and the block edge, a system whose matrices run through the length-class lists
and the alias rows, tiled systems, NULL outputs, the extents written, out-of-range witnesses, the checked proof, and the path from the
given rows of a batch to the list of its bad copies.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_ref as ref
import c_oracle as co
import fixtures as fx
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import check as K
from fawkes_crypto_amd import witness as W
from helpers import r1cs_product, TOXIC
import check_cases as cc
from test_gpu_spmv_dedup import crafted_system, alias_table, random_z, knobs  # noqa: F401  (knobs: a fixture)
from test_gpu_witness import Gadget, _BUILD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ref.R
TOX = {k: fx.mont_fr(v) for k, v in TOXIC.items()}
MARK64, MARK8 = 0xa5a5a5a5a5a5a5a5, 0x5a


def fields(rep):
    """a CheckReport as a comparable tuple: every field, the bitmap, the flags"""
    return (rep.gates, rep.n_bad, rep.first_bad, rep.first_abc_mont.tobytes(), rep.first_abc, rep.n_groups, rep.n_bad_groups, rep.n_range,
            rep.first_range, rep.one_ok, rep.gates_valid, rep.ok, rep.bitmap().tobytes(), rep.bad_rows().tolist(),
            rep.group_flags().tobytes() if rep.group_rows else None)


def both(ctx, dr, prod, z, copies=1, group_rows=None, want=None):
    """device == host reference (== the oracle's expectation, where given); returns the device report"""
    dev = K.check_witness(ctx, dr, z, group_rows=group_rows)
    host = K.check_host(prod, z, copies=copies, group_rows=group_rows)
    assert fields(dev) == fields(host)
    if want is not None:
        cc.assert_report(dev, want)
    return dev


# ---------------------------------------------------------------- explicit systems
@pytest.mark.parametrize('gates', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_explicit_system(ctx, gates):
    csr, z = cc.explicit_case(gates)
    prod = r1cs_product(csr)
    dr = ctx.load_r1cs(prod)
    try:
        rep = both(ctx, dr, prod, z, group_rows=7, want=cc.Want(csr, z, 7))
        assert rep.ok and rep.n_bad == 0 and rep.first_bad is None
        for k, bad in enumerate(cc.bad_sets(gates)):
            zb = cc.violate(csr, z, bad, seed=gates + k)
            w = cc.Want(csr, zb, 7)
            assert set(bad) <= set(w.bad)
            both(ctx, dr, prod, zb, group_rows=7, want=w)
            both(ctx, dr, prod, zb, want=w.regroup(0))
        za = cc.all_bad(csr, z)
        rep = both(ctx, dr, prod, za, group_rows=64, want=cc.Want(csr, za, 64))
        assert rep.n_bad == gates
    finally:
        dr.free()


# ---------------------------------------------------------------- length-class lists and alias rows
def test_class_lists_and_alias_rows(ctx, knobs):
    """A and B of tests/test_gpu_spmv_dedup.py's crafted system (rows of up to 512 terms: the length-class lists; repeated rows: the alias
    plan) with C rebuilt as one term per gate, c_g * ONE, so that a random witness satisfies it: C stays on the plain kernel.  Violations
    are placed on a variable that a source row and its alias two gates on both read."""
    min_len, back = knobs
    base, _, _, _ = crafted_system(min_len, back, c_short=True)
    gates = base.num_gates
    z = random_z(base.num_input + base.num_aux, 5)
    a, b, _ = (x[:gates] for x in co.synthesize(base, z)[:3])
    seq = np.arange(gates + 1, dtype=np.uint64)
    csr = co.R1csC(base.num_input, base.num_aux, base.A, base.B, co.Csr(seq, np.zeros(gates, np.uint32), co.fe_mul_batch(co.FR, a, b)))
    assert cc.Want(csr, z).n_bad == 0
    prod = r1cs_product(csr)
    dr = ctx.load_r1cs(prod)
    try:
        table = alias_table(dr)
        assert table and max(int(np.diff(m.ptr.astype(np.int64)).max()) for m in (csr.A, csr.B)) >= 8
        both(ctx, dr, prod, z, group_rows=100, want=cc.Want(csr, z, 100))
        dm, drow, sm, srow = next(t for t in table if t[1] != t[3])          # e.g. B row g + 2 = A row g
        src = (csr.A, csr.B, csr.C)[sm]
        v = next(int(c) for c in src.col[int(src.ptr[srow]):int(src.ptr[srow + 1])] if c)
        zb = z.copy(); zb[v] = fx.mont_fr(0x1234567)
        w = cc.Want(csr, zb, 100)
        assert {srow, drow} <= set(w.bad)                                    # the source's gate and the alias's
        both(ctx, dr, prod, zb, group_rows=100, want=w)
        # ... and an alias in the same gate as its source
        dm, drow, sm, srow = next(t for t in table if t[1] == t[3])
        src = (csr.A, csr.B, csr.C)[sm]
        v = next(int(c) for c in src.col[int(src.ptr[srow]):int(src.ptr[srow + 1])] if c)
        zb = z.copy(); zb[v] = fx.mont_fr(0x7654321)
        w = cc.Want(csr, zb, 1)
        assert drow in w.bad
        both(ctx, dr, prod, zb, group_rows=1, want=w)
    finally:
        dr.free()


# ---------------------------------------------------------------- tiled systems
@pytest.mark.parametrize('G,copies', [(5, 1), (5, 70), (37, 64), (37, 65), (100, 130)])
def test_tiled_system(ctx, G, copies):
    inst, full, z = cc.tiled_case(G, copies)
    prod = r1cs_product(inst)
    dr = ctx.load_r1cs(prod, copies=copies)
    try:
        cases = [[], [0], [copies - 1], list(range(copies))]
        if copies > 64:
            cases.append([63, 64])
        for altered in cases:
            zb = cc.violate_copies(inst, full, z, altered) if altered else z
            w = cc.Want(full, zb, G)
            rep = both(ctx, dr, prod, zb, copies=copies, group_rows=G, want=w)
            assert rep.bad_groups().tolist() == sorted(set(altered))
            for gr in cc.GROUP_ROWS:
                both(ctx, dr, prod, zb, copies=copies, group_rows=gr, want=w.regroup(gr))
    finally:
        dr.free()


# ---------------------------------------------------------------- NULL outputs, extents, the witness untouched
def _raw_dev(ctx, dr, d_z, group_rows, d_bitmap, d_flags):
    st = K.CheckReportStruct()
    ctx._ck(K._lib().fk_r1cs_check_dev(ctx.handle, dr.handle, d_z, group_rows, d_bitmap, d_flags, C.byref(st)))
    return cc.struct_fields(st)


@pytest.mark.parametrize('gates,group_rows', [(257, 7), (1000, 64), (64, 1)])
def test_null_outputs_and_extents(ctx, gates, group_rows):
    csr, z = cc.explicit_case(gates)
    zb = cc.violate(csr, z, [0, gates - 1], seed=gates)
    w = cc.Want(csr, zb, group_rows)
    dr = ctx.load_r1cs(r1cs_product(csr))
    words, groups = len(w.bitmap), w.n_groups
    d_z, d_bm, d_fl = ctx.dev_alloc(zb.nbytes), ctx.dev_alloc(8 * (words + 4)), ctx.dev_alloc(groups + 16)
    try:
        ctx.upload(d_z, zb)
        ctx.upload(d_bm, np.full(words + 4, MARK64, np.uint64))
        ctx.upload(d_fl, np.full(groups + 16, MARK8, np.uint8))
        full = _raw_dev(ctx, dr, d_z, group_rows, d_bm, d_fl)
        assert full == cc.want_fields(w)
        bm, fl = ctx.download(d_bm, 8 * (words + 4), np.uint64), ctx.download(d_fl, groups + 16, np.uint8)
        assert np.array_equal(bm[:words], w.bitmap) and (bm[words:] == MARK64).all()            # marker words behind the bitmap
        assert np.array_equal(fl[:groups], w.flags) and (fl[groups:] == MARK8).all()            # ... and behind the flags
        # NULL bitmap, NULL flags, both NULL: the same report, and an array that was not passed is not written
        ctx.upload(d_bm, np.full(words + 4, MARK64, np.uint64))
        ctx.upload(d_fl, np.full(groups + 16, MARK8, np.uint8))
        assert _raw_dev(ctx, dr, d_z, group_rows, None, d_fl) == full
        assert (ctx.download(d_bm, 8 * (words + 4), np.uint64) == MARK64).all()
        assert np.array_equal(ctx.download(d_fl, groups, np.uint8), w.flags)
        ctx.upload(d_fl, np.full(groups + 16, MARK8, np.uint8))
        assert _raw_dev(ctx, dr, d_z, group_rows, d_bm, None) == full
        assert (ctx.download(d_fl, groups + 16, np.uint8) == MARK8).all()
        assert np.array_equal(ctx.download(d_bm, 8 * words, np.uint64), w.bitmap)
        assert _raw_dev(ctx, dr, d_z, group_rows, None, None) == full
        assert _raw_dev(ctx, dr, d_z, 0, None, None) == cc.want_fields(w.regroup(0))
        assert np.array_equal(ctx.download(d_z, zb.nbytes, np.uint64).reshape(-1, 4), zb)       # the witness is only read
    finally:
        for p in (d_z, d_bm, d_fl):
            ctx.dev_free(p)
        dr.free()


def test_errors(ctx):
    csr, z = cc.explicit_case(65)
    dr = ctx.load_r1cs(r1cs_product(csr))
    d_z, d_fl = ctx.dev_alloc(z.nbytes), ctx.dev_alloc(128)
    lib = K._lib()
    st = K.CheckReportStruct()
    try:
        ctx.upload(d_z, z)
        assert lib.fk_r1cs_check_dev(ctx.handle, dr.handle, d_z, 0, None, None, None) == 1
        assert lib.fk_r1cs_check_dev(ctx.handle, None, d_z, 0, None, None, C.byref(st)) == 1
        assert lib.fk_r1cs_check_dev(ctx.handle, dr.handle, None, 0, None, None, C.byref(st)) == 1
        assert lib.fk_r1cs_check_dev(ctx.handle, dr.handle, d_z, 0, None, d_fl, C.byref(st)) == 1
        assert lib.fk_r1cs_check_dev(ctx.handle, dr.handle, d_z, 1, None, d_fl, C.byref(st)) == 0 and st.n_bad == 0 and st.n_groups == 65
        with pytest.raises(fk.FkError):              # a host witness of another length
            K.check_witness(ctx, dr, z[:-1])
    finally:
        ctx.dev_free(d_z); ctx.dev_free(d_fl)
        dr.free()


# ---------------------------------------------------------------- range
def test_range(ctx):
    csr, z = cc.explicit_case(300)
    prod = r1cs_product(csr)
    dr = ctx.load_r1cs(prod)
    nv = len(z)

    def spec(rep):
        return (rep.gates, rep.n_groups, rep.n_range, rep.first_range, rep.one_ok, rep.gates_valid, rep.ok)

    try:
        zr = z.copy(); zr[nv - 1] = fk.api.int_to_limbs(R)                       # r itself at the last index
        dev, host = K.check_witness(ctx, dr, zr, group_rows=8), K.check_host(prod, zr, group_rows=8)
        assert spec(dev) == spec(host) == (300, 38, 1, nv - 1, True, False, False)
        zr[nv // 2] = fk.api.int_to_limbs((1 << 256) - 1)                        # 2^256 - 1 in the middle
        dev, host = K.check_witness(ctx, dr, zr), K.check_host(prod, zr)
        assert spec(dev) == spec(host) == (300, 0, 2, nv // 2, True, False, False)
        zr = z.copy(); zr[nv - 1] = fk.api.int_to_limbs(R - 1)                   # r - 1 is in range
        rep = both(ctx, dr, prod, zr, want=cc.Want(csr, zr))
        assert rep.gates_valid and rep.n_range == 0
        z0 = z.copy(); z0[0] = 0                                                 # not ONE, in range: the gates are judged
        rep = both(ctx, dr, prod, z0, group_rows=8, want=cc.Want(csr, z0, 8))
        assert (rep.one_ok, rep.n_range, rep.gates_valid, rep.ok) == (False, 0, True, False)
    finally:
        dr.free()


# ---------------------------------------------------------------- the checked proof
@pytest.fixture(scope='module')
def proving(ctx):
    """a small set-up system: (R1csC, R1cs, key, resident system, satisfying witness, violated witness)"""
    csr, z = cc.explicit_case(300, seed=77)
    prod = r1cs_product(csr)
    dk, _ = ctx.setup(prod, **TOX)
    dr = ctx.load_r1cs(prod)
    zb = cc.violate(csr, z, [0, 64, 299], seed=5)
    yield csr, prod, dk, dr, z, zb
    dr.free(); dk.free()


def test_checked_proof(ctx, proving):
    csr, prod, dk, dr, z, zb = proving
    r, s = fx.mont_fr(0x5eed), fx.mont_fr(0xfeed)
    d_z = ctx.dev_alloc(z.nbytes)
    try:
        # a submit / wait pair run before the checked call leaves it working
        pin = ctx.host_alloc((len(z), 4))
        pin[:] = z
        piped = ctx.prove_witness_wait(ctx.prove_witness_submit(dk, dr, pin, r, s))
        ctx.host_free(pin)
        for wit in (z, zb):
            ctx.upload(d_z, wit)
            plain = ctx.prove_witness_dev(dk, dr, d_z, r, s)
            proof, rep = K.prove_checked(ctx, dk, dr, d_z, r, s, group_rows=7)
            assert proof.tobytes() == plain.tobytes() and len(proof.tobytes()) == 256
            assert fields(rep) == fields(K.check_witness(ctx, dr, d_z, group_rows=7)) == fields(K.check_host(prod, wit, group_rows=7))
            cc.assert_report(rep, cc.Want(csr, wit, 7))
            assert ctx.prove_witness_dev(dk, dr, d_z, r, s).tobytes() == plain.tobytes()      # a following plain proof
            proof2, rep2, tm = K.prove_checked(ctx, dk, dr, d_z, r, s, want_timings=True)      # without groups
            assert proof2.tobytes() == plain.tobytes() and fields(rep2) == fields(K.check_host(prod, wit)) and isinstance(tm, dict)
            assert np.array_equal(ctx.download(d_z, wit.nbytes, np.uint64).reshape(-1, 4), wit)
            if wit is z:
                assert rep.ok and piped.tobytes() == plain.tobytes()
            else:
                assert not rep.ok and {0, 64, 299} <= set(rep.bad_rows().tolist())
                with pytest.raises(K.Unsatisfied) as e:
                    K.prove_checked(ctx, dk, dr, d_z, r, s, group_rows=7, raise_on_bad=True)
                assert e.value.proof.tobytes() == plain.tobytes() and fields(e.value.report) == fields(rep)
        ctx.upload(d_z, z)
        assert K.prove_checked(ctx, dk, dr, d_z, r, s, raise_on_bad=True)[1].ok
    finally:
        ctx.dev_free(d_z)


def test_checked_proof_reports_mismatches_as_the_plain_one(ctx, proving):
    csr, prod, dk, dr, z, _ = proving
    other, z2 = cc.explicit_case(65)
    dr2 = ctx.load_r1cs(r1cs_product(other))
    r, s = fx.mont_fr(1), fx.mont_fr(2)
    d_z = ctx.dev_alloc(max(z.nbytes, z2.nbytes))
    lib = K._lib()
    try:
        ctx.upload(d_z, z2)
        with pytest.raises(fk.FkError) as plain:
            ctx.prove_witness_dev(dk, dr2, d_z, r, s)
        with pytest.raises(fk.FkError) as checked:
            K.prove_checked(ctx, dk, dr2, d_z, r, s)
        assert checked.value.code == plain.value.code == 6 and str(checked.value) == str(plain.value)
        st, out = K.CheckReportStruct(), np.zeros(256, np.uint8)
        rp, sp = r.ctypes.data, s.ctypes.data
        args = (rp, sp, out.ctypes.data, None, 0, None, None)
        assert lib.fk_prove_r1cs_checked_dev(ctx.handle, dk.handle, dr.handle, d_z, *args, None) == 1          # null report
        assert lib.fk_prove_r1cs_checked_dev(ctx.handle, None, dr.handle, d_z, *args, C.byref(st)) == 1
        assert lib.fk_prove_r1cs_checked_dev(ctx.handle, dk.handle, None, d_z, *args, C.byref(st)) == 1
        assert lib.fk_prove_r1cs_checked_dev(ctx.handle, dk.handle, dr.handle, None, *args, C.byref(st)) == 1
        assert lib.fk_prove_r1cs_checked_dev(ctx.handle, dk.handle, dr.handle, d_z, rp, sp, out.ctypes.data, None, 0, None, d_z, C.byref(st)) == 1     # flags without group_rows
        ctx.upload(d_z, z)
        assert K.prove_checked(ctx, dk, dr, d_z, r, s)[1].ok                     # the context is as it was
    finally:
        ctx.dev_free(d_z)
        dr2.free()


def test_an_outstanding_early_front_is_refused():
    """the early front exists under the sorts-first schedule only, which is chosen per process: tests/_check_child.py"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(('FK_SPMV_', 'FK_PROVE_'))}
    env['FK_PROVE_SORTS_FIRST'] = '1'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_check_child.py')], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'CHECK ok early_front_refused=True' in out.stdout, out.stdout[-1000:]


# ---------------------------------------------------------------- end to end: given rows -> witness -> checked proof -> bad copies
def test_given_rows_to_bad_copies(ctx):
    copies, wrong = 65, [0, 33, 64]
    g = Gadget(*_BUILD['merkle2'])
    dp = W.load(ctx, g.prog)
    dk, vk = ctx.setup(g.r1cs, copies=copies, **TOX)
    dr = ctx.load_r1cs(g.r1cs, copies=copies)
    vkb = fk.vk_to_borsh(vk)
    r, s = fx.mont_fr(0xabc), fx.mont_fr(0xdef)
    G, ni = g.num_gates, g.prog.num_input
    try:
        good = [list(g.given[k % 3]) for k in range(copies)]
        bad = [list(row) for row in good]
        for k in wrong:
            bad[k][0] = (bad[k][0] + 1) % R                                      # the root this copy claims
        for rows, expect in ((good, []), (bad, wrong)):
            z = W.generate(ctx, dp, rows)
            proof, rep = K.prove_given_checked(ctx, dk, dr, dp, rows, r, s)
            assert proof.tobytes() == W.prove_given(ctx, dk, dr, dp, rows, r, s).tobytes()
            assert rep.gates == copies * G and rep.n_groups == copies and rep.gates_valid and rep.one_ok
            assert rep.bad_groups().tolist() == expect and rep.n_bad_groups == len(expect)
            assert fields(rep) == fields(K.check_host(g.r1cs, z, copies=copies, group_rows=G))
            assert fk.api.verify(vkb, z[1:1 + copies * (ni - 1)], proof.tobytes(), ctx) == (not expect)
            if expect:
                assert not rep.ok and 0 <= rep.first_bad < G
                assert {int(x) // G for x in rep.bad_rows()} == set(expect)
                with pytest.raises(K.Unsatisfied):
                    K.prove_given_checked(ctx, dk, dr, dp, rows, r, s, raise_on_bad=True)
            else:
                assert rep.ok and rep.first_bad is None
    finally:
        dr.free(); dk.free(); dp.free()
