"""The R1CS check on the host (no GPU): fk_r1cs_check through fawkes_crypto_amd/check.py against what the oracle says (`c_oracle.synthesize`
plus `fe_mul_batch`, tests/check_cases.py) on satisfied, violated, tiled and out-of-range witnesses; its refusals and the extents it writes;
and include/fawkes_hip_check.h against the library and the ctypes table.  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bn254_ref as ref
import fixtures as fx
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import check as K
from helpers import r1cs_product
import check_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'fawkes_hip_check.h')
FK_ERR_BAD_ARG = 1
R = ref.R


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


def test_header_compiles_alone_as_c99():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include "fawkes_hip_check.h"\nint main(void) { fk_check_report r; r.first_bad = FK_CHECK_NONE; return r.first_bad + 1 == 0 ? 0 : 1; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(K.PROTOTYPES) and len(decl) == 3
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(K.PROTOTYPES[name][1]) == nargs, name
    # kept out of the pinned ABI
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    assert 'FK_CHECK' not in open(os.path.join(ROOT, 'include', 'fawkes_hip.h')).read()


def test_report_layout_c_vs_ctypes():
    fields = [f[0] for f in K.CheckReportStruct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "fawkes_hip_check.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fk_check_report));']
    prog += ['  printf("%s %%zu\\n", offsetof(fk_check_report, %s));' % (f, f) for f in fields]
    prog += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, 'layout.c'), os.path.join(td, 'layout')
        open(src, 'w').write('\n'.join(prog))
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got.pop('size')) == C.sizeof(K.CheckReportStruct) == 160
    assert {f: int(v) for f, v in got.items()} == {f: getattr(K.CheckReportStruct, f).offset for f in fields}
    assert K.CHECK_NONE == cc.NONE


# ---------------------------------------------------------------- explicit systems
@pytest.mark.parametrize('gates', [1, 63, 64, 65, 300])
def test_satisfied_system(gates):
    csr, z = cc.explicit_case(gates)
    w = cc.Want(csr, z, 7)
    assert w.n_bad == 0
    rep = K.check_host(r1cs_product(csr), z, group_rows=7)
    cc.assert_report(rep, w)
    assert rep.ok and rep.first_bad is None and not rep.bitmap().any() and not rep.first_abc_mont.any() and rep.n_bad_groups == 0


@pytest.mark.parametrize('gates', [1, 63, 64, 65, 300])
def test_violated_system(gates):
    csr, z = cc.explicit_case(gates)
    prod = r1cs_product(csr)
    for k, bad in enumerate(cc.bad_sets(gates)):
        zb = cc.violate(csr, z, bad, seed=gates + k)
        w = cc.Want(csr, zb, 7)
        assert set(bad) <= set(w.bad)
        cc.assert_report(K.check_host(prod, zb, group_rows=7), w)
        cc.assert_report(K.check_host(prod, zb), w.regroup(0))
    za = cc.all_bad(csr, z)
    w = cc.Want(csr, za, 64)
    assert w.n_bad == gates and w.first_bad == 0
    cc.assert_report(K.check_host(prod, za, group_rows=64), w)


# ---------------------------------------------------------------- the tiled reference
@pytest.mark.parametrize('G,copies', [(5, 1), (5, 70), (37, 65)])
def test_tiled_reference_equals_the_explicit_system(G, copies):
    inst, full, z = cc.tiled_case(G, copies)
    p_inst, p_full = r1cs_product(inst), r1cs_product(full)
    assert full.num_gates == G * copies
    for altered in ([], [0], [copies - 1], sorted({0, copies // 2, copies - 1}), list(range(copies))):
        zb = cc.violate_copies(inst, full, z, altered) if altered else z
        w = cc.Want(full, zb, G)
        assert [int(k) for k in np.flatnonzero(w.flags)] == altered
        cc.assert_report(K.check_host(p_inst, zb, copies=copies, group_rows=G), w)
        cc.assert_report(K.check_host(p_full, zb, group_rows=G), w)
        for gr in (1, 64, G * copies + 5):
            cc.assert_report(K.check_host(p_inst, zb, copies=copies, group_rows=gr), w.regroup(gr))


# ---------------------------------------------------------------- range
def _raw(prod, z, copies=1, group_rows=0, words=None, groups=None):
    """fk_r1cs_check called directly: (rc, report struct, bitmap with 4 guard words, flags with 16 guard bytes)"""
    gates = prod.num_gates * max(copies, 1)
    words = (gates + 63) // 64 if words is None else words
    groups = ((gates + group_rows - 1) // group_rows if group_rows else 0) if groups is None else groups
    bitmap = np.full(words + 4, 0xa5a5a5a5a5a5a5a5, np.uint64)
    flags = np.full(groups + 16, 0x5a, np.uint8)
    st = K.CheckReportStruct()
    rc = K._lib().fk_r1cs_check(None, C.byref(prod.struct), copies, z.ctypes.data, group_rows, bitmap.ctypes.data, flags.ctypes.data if group_rows else None, C.byref(st))
    return rc, st, bitmap, flags


def test_range():
    csr, z = cc.explicit_case(65)
    prod = r1cs_product(csr)
    nv = len(z)
    # r itself at the last index
    zr = z.copy(); zr[nv - 1] = fk.api.int_to_limbs(R)
    rep = K.check_host(prod, zr, group_rows=8)
    assert (rep.n_range, rep.first_range, rep.gates_valid, rep.one_ok, rep.ok) == (1, nv - 1, False, True, False)
    assert (rep.gates, rep.n_groups) == (65, 9)
    # 2^256 - 1 in the middle, r at the end: two, the lowest named
    zr[nv // 2] = fk.api.int_to_limbs((1 << 256) - 1)
    rep = K.check_host(prod, zr)
    assert (rep.n_range, rep.first_range, rep.gates_valid) == (2, nv // 2, False)
    # r - 1 is in range
    zr = z.copy(); zr[nv - 1] = fk.api.int_to_limbs(R - 1)
    rep = K.check_host(prod, zr)
    assert (rep.n_range, rep.first_range, rep.gates_valid) == (0, None, True)
    cc.assert_report(rep, cc.Want(csr, zr))
    # z[0] = 0: in range, not ONE; the gates are judged as the oracle judges them
    z0 = z.copy(); z0[0] = 0
    rep = K.check_host(prod, z0, group_rows=8)
    assert (rep.one_ok, rep.n_range, rep.gates_valid, rep.ok) == (False, 0, True, False)
    cc.assert_report(rep, cc.Want(csr, z0, 8))
    # out of range: the arrays are still written inside their extents only
    zr = z.copy(); zr[3] = fk.api.int_to_limbs(R + 5)
    rc, st, bitmap, flags = _raw(prod, zr, group_rows=8)
    assert rc == 0 and (st.n_range, st.first_range, st.gates_valid) == (1, 3, 0)
    assert (bitmap[2:] == 0xa5a5a5a5a5a5a5a5).all() and (flags[9:] == 0x5a).all()


# ---------------------------------------------------------------- errors and extents
def test_errors():
    csr, z = cc.explicit_case(65)
    prod = r1cs_product(csr)
    lib = K._lib()
    st = K.CheckReportStruct()
    bitmap, flags = np.zeros(2, np.uint64), np.zeros(65, np.uint8)
    args = dict(cs=C.byref(prod.struct), copies=1, z=z.ctypes.data, group_rows=0, bitmap=bitmap.ctypes.data, flags=None, rep=C.byref(st))

    def call(**kw):
        a = dict(args, **kw)
        return lib.fk_r1cs_check(None, a['cs'], a['copies'], a['z'], a['group_rows'], a['bitmap'], a['flags'], a['rep'])

    assert call() == 0
    assert call(rep=None) == FK_ERR_BAD_ARG
    assert call(cs=None) == FK_ERR_BAD_ARG
    assert call(z=None) == FK_ERR_BAD_ARG
    assert call(copies=0) == FK_ERR_BAD_ARG
    assert call(flags=flags.ctypes.data, group_rows=0) == FK_ERR_BAD_ARG
    assert b'group_rows' in lib.fk_last_error(None)
    assert call(flags=flags.ctypes.data, group_rows=1) == 0
    assert call(bitmap=None, flags=None, group_rows=3) == 0 and st.n_groups == 22          # both arrays are optional
    with pytest.raises(fk.FkError) as e:
        K.check_host(prod, z, copies=0)
    assert e.value.code == FK_ERR_BAD_ARG
    with pytest.raises(fk.FkError):                  # a witness of another length than the copies need
        K.check_host(prod, z, copies=2)


@pytest.mark.parametrize('gates,group_rows', [(63, 1), (64, 64), (65, 7), (300, 301)])
def test_guard_bytes_behind_the_bitmap_and_the_flags(gates, group_rows):
    csr, z = cc.explicit_case(gates)
    prod = r1cs_product(csr)
    za = cc.all_bad(csr, z)
    w = cc.Want(csr, za, group_rows)
    rc, st, bitmap, flags = _raw(prod, za, group_rows=group_rows)
    assert rc == 0 and cc.struct_fields(st) == cc.want_fields(w)
    assert np.array_equal(bitmap[:-4], w.bitmap) and (bitmap[-4:] == 0xa5a5a5a5a5a5a5a5).all()
    assert np.array_equal(flags[:-16], w.flags) and (flags[-16:] == 0x5a).all()
    # the bits at and beyond `gates` are zero
    if gates % 64:
        assert int(bitmap[len(w.bitmap) - 1]) >> (gates % 64) == 0
