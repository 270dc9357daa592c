"""The batch prover's R1CS check on the host (no GPU): fk_batch_r1cs_check against what the oracle says of every proof on its own
(`check_cases.Want`: `c_oracle.synthesize` plus `fe_mul_batch`), field by field with bitmap and flags, in both witness layouts; against
fk_r1cs_check one proof at a time; out-of-range witnesses and wrong ONEs; refusals and extents; and include/fawkes_hip_batch_check.h
against the library and the ctypes table.  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import batch as B
from fawkes_crypto_amd import check as K
from helpers import r1cs_product
import check_cases as cc
from batch_cases import tile_rows
from batch_check_cases import GATES, LAYOUTS, laid_out, range_cases, range_system, variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'fawkes_hip_batch_check.h')
FK_ERR_BAD_ARG = 1
R = ref.R
COUNTS = (1, 3)
GUARD = 0xa5a5a5a5a5a5a5a5


@pytest.fixture(scope='module', autouse=True)
def _oracle(oracle):
    return oracle


def raw(prod, z, layout, count, words=None):
    """fk_batch_r1cs_check called directly: (rc, report structs, bitmap (count, words) behind and in front of 4 guard words, flags
    behind and in front of 16 guard bytes)"""
    words = (prod.num_gates + 63) // 64 if words is None else words
    bitmap = np.full(count * words + 8, GUARD, np.uint64)
    flags = np.full(count + 32, 0x5a, np.uint8)
    sts = (K.CheckReportStruct * max(count, 1))()
    rc = B._lib().fk_batch_r1cs_check(None, C.byref(prod.struct), z.ctypes.data, layout, count, bitmap[4:].ctypes.data, flags[16:].ctypes.data, sts)
    assert (bitmap[:4] == GUARD).all() and (bitmap[4 + count * words:] == GUARD).all(), 'the bitmap was written outside its extent'
    assert (flags[:16] == 0x5a).all() and (flags[16 + count:] == 0x5a).all(), 'the flags were written outside their extent'
    return rc, list(sts)[:count], bitmap[4:4 + count * words].reshape(count, words), flags[16:16 + count]


def assert_proof(st, bitmap, flag, w, where):
    """one proof's report, bitmap row and flag against the oracle's expectation"""
    assert cc.struct_fields(st) == cc.want_fields(w), where
    assert np.array_equal(bitmap, w.bitmap), where
    assert int(flag) == int(w.n_bad > 0 or not w.one_ok), where


# ---------------------------------------------------------------- the header, the library, the ctypes table
def _declared():
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b(fk_\w+)\s*\(([^()]*)\)\s*;', text):
        out[name] = len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])
    return out


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(B.CHECK_PROTOTYPES) and len(decl) == 4
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(B.CHECK_PROTOTYPES[name][1]) == nargs, name
    # kept out of the pinned ABI, and out of the table that mirrors fawkes_hip_batch.h
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    assert not set(decl) & set(B.PROTOTYPES)


def test_header_compiles_alone_as_c99_and_the_constants_agree():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include "fawkes_hip_batch_check.h"\nint main(void) { fk_check_report r; fk_batch_opts o; (void)o; r.first_bad = FK_CHECK_NONE; '
                             'return r.first_bad + 1 == 0 && FK_BATCH_CHECK_LAUNCHES == %d && FK_BATCH_CHECK_RECORD_BYTES == %d '
                             '&& sizeof(fk_check_report) == FK_BATCH_CHECK_RECORD_BYTES && FK_BATCH_Z_TILED == %d ? 0 : 1; }\n'
                             % (B.CHECK_LAUNCHES, B.CHECK_RECORD_BYTES, B.Z_TILED))
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-Wno-long-long', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])
    assert C.sizeof(K.CheckReportStruct) == B.CHECK_RECORD_BYTES


# ---------------------------------------------------------------- gates
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('gates', GATES)
def test_every_proof_is_reported_as_the_oracle_judges_it(gates, count, layout):
    """every variant (satisfied, each bad set, all bad) stands at every place of a batch: windows of `count` consecutive variants"""
    csr, prod, var = variants(gates)
    for k in range(len(var)):
        pick = [var[(k + i) % len(var)] for i in range(count)]
        z = laid_out([x for x, _ in pick], layout, csr.num_input)
        rc, sts, bitmap, flags = raw(prod, z, layout, count)
        assert rc == 0
        for i, (_, w) in enumerate(pick):
            assert_proof(sts[i], bitmap[i], flags[i], w, (gates, count, layout, k, i))
            if gates % 64:
                assert int(bitmap[i][-1]) >> (gates % 64) == 0          # the bits at and beyond `gates` are zero


@pytest.mark.parametrize('gates', GATES)
def test_one_proof_at_a_time_through_fk_r1cs_check_gives_the_same_fields(gates):
    csr, prod, var = variants(gates)
    zs = [x for x, _ in var]
    words = (gates + 63) // 64
    for layout in LAYOUTS:
        rc, sts, bitmap, _ = raw(prod, laid_out(zs, layout, csr.num_input), layout, len(zs))
        assert rc == 0
        for i, z in enumerate(zs):
            one, bm = K.CheckReportStruct(), np.zeros(words, np.uint64)
            assert K._lib().fk_r1cs_check(None, C.byref(prod.struct), 1, z.ctypes.data, 0, bm.ctypes.data, None, C.byref(one)) == 0
            assert cc.struct_fields(sts[i]) == cc.struct_fields(one), (gates, layout, i)
            assert np.array_equal(bitmap[i], bm), (gates, layout, i)


def test_python_wrapper_returns_check_reports():
    csr, prod, var = variants(65)
    zs = np.stack([x for x, _ in var])
    for reps in (B.check_batch_host(prod, zs), B.check_batch_host(prod, tile_rows(list(zs), csr.num_input), layout=B.Z_TILED)):
        assert len(reps) == len(var)
        for rep, (_, w) in zip(reps, var):
            cc.assert_report(rep, w)
    assert B.check_batch_host(prod, zs[:0]) == []
    with pytest.raises(fk.FkError):                  # a length that is no whole number of witnesses
        B.check_batch_host(prod, np.concatenate(list(zs))[:-1], count=len(zs))


# ---------------------------------------------------------------- range and ONE
def assert_range_case(csr, zs, expect, sts, bitmap, flags, where):
    for i, (z, diff) in enumerate(zip(zs, expect)):
        if diff is None:
            assert_proof(sts[i], bitmap[i], flags[i], cc.Want(csr, z), (where, i))
            continue
        assert cc.struct_fields(sts[i]) == diff, (where, i)
        assert not bitmap[i].any() and flags[i] == 1, (where, i)


def test_range_and_one():
    csr, prod, z = range_system()
    cases = range_cases(csr, z)
    for (name, layout), (zs, expect) in cases.items():
        rc, sts, bitmap, flags = raw(prod, laid_out(zs, layout, csr.num_input), layout, 3)
        assert rc == 0
        assert_range_case(csr, zs, expect, sts, bitmap, flags, (name, layout))
    # what the cases are there for
    _, sts, _, flags = raw(prod, laid_out(cases['a wrong ONE in one row', B.Z_ROWS][0], B.Z_ROWS, 3), B.Z_ROWS, 3)
    assert [st.one_ok for st in sts] == [1, 0, 1] and list(flags) == [1, 1, 0]
    _, sts, _, flags = raw(prod, laid_out(cases['a wrong shared ONE', B.Z_TILED][0], B.Z_TILED, 3), B.Z_TILED, 3)
    assert [st.one_ok for st in sts] == [0, 0, 0] and [st.n_range for st in sts] == [0, 0, 0] and list(flags) == [1, 1, 1]
    _, sts, _, _ = raw(prod, laid_out(cases['r at variable 1 of proof 1', B.Z_TILED][0], B.Z_TILED, 3), B.Z_TILED, 3)
    assert [st.gates_valid for st in sts] == [1, 0, 1] and sts[0].n_bad > 0 and sts[2].n_bad == 0


# ---------------------------------------------------------------- refusals, the empty call, optional outputs
def test_refusals_and_the_empty_call():
    csr, prod, var = variants(65)
    z = laid_out([x for x, _ in var[:3]], B.Z_ROWS, csr.num_input)
    lib = B._lib()
    sts = (K.CheckReportStruct * 3)()
    bitmap, flags = np.full(6, GUARD, np.uint64), np.full(3, 0x5a, np.uint8)
    args = dict(cs=C.byref(prod.struct), z=z.ctypes.data, layout=B.Z_ROWS, count=3, bitmap=bitmap.ctypes.data, flags=flags.ctypes.data, reps=sts)

    def call(**kw):
        a = dict(args, **kw)
        return lib.fk_batch_r1cs_check(None, a['cs'], a['z'], a['layout'], a['count'], a['bitmap'], a['flags'], a['reps'])

    assert call(reps=None) == FK_ERR_BAD_ARG and b'null' in lib.fk_last_error(None)
    assert call(cs=None) == FK_ERR_BAD_ARG
    assert call(z=None) == FK_ERR_BAD_ARG
    assert call(layout=2) == FK_ERR_BAD_ARG and b'layout' in lib.fk_last_error(None)
    # count == 0: FK_OK whatever else is null, nothing written
    assert call(count=0) == 0 and call(count=0, reps=None, z=None, cs=None) == 0
    assert (bitmap == GUARD).all() and (flags == 0x5a).all() and bytes(sts) == bytes(C.sizeof(sts))
    # both arrays are optional
    assert call(bitmap=None, flags=None) == 0
    assert [cc.struct_fields(st) for st in sts] == [cc.want_fields(w) for _, w in var[:3]]
    assert (bitmap == GUARD).all() and (flags == 0x5a).all()
    assert call() == 0 and np.array_equal(bitmap.reshape(3, 2), np.stack([w.bitmap for _, w in var[:3]]))
