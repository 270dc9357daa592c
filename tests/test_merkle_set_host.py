"""The bulk leaf writes without a GPU: include/fawkes_hip_merkle_set.h against the library and the ctypes table of
fawkes_crypto_amd/merkle_set.py, that the six entries stay out of the pinned ABI and out of the two older headers and tables, the
package export, and the refusals that need no device."""
import os
import re
import subprocess
import tempfile

import numpy as np

import fawkes_crypto_amd as fk
from fawkes_crypto_amd import merkle as M
from fawkes_crypto_amd import merkle_set as MS
from fawkes_crypto_amd import sparse_merkle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
HEADER = os.path.join(INCLUDE, 'fawkes_hip_merkle_set.h')
FK_ERR_BAD_ARG = 1
MARK = 0xa5a5a5a5a5a5a5a5


def _declared():
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b(fk_\w+)\s*\(([^()]*)\)\s*;', text):
        out[name] = len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])
    return out


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(MS.PROTOTYPES) and len(decl) == 6
    assert decl['fk_smt_set_dev'] == decl['fk_smt_set'] == 6 and decl['fk_smt_set_timed_dev'] == 8
    assert decl['fk_poseidon_merkle_set_dev'] == decl['fk_poseidon_merkle_set'] == 7 and decl['fk_poseidon_merkle_set_timed_dev'] == 9
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(MS.PROTOTYPES[name][1]) == nargs, name


def test_the_entries_stay_out_of_the_pinned_abi_and_of_the_older_headers():
    decl = _declared()
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    assert not set(decl) & set(S.PROTOTYPES) and not set(decl) & set(M.PROTOTYPES)
    pinned = open(os.path.join(INCLUDE, 'fawkes_hip.h')).read()
    assert not any(n in pinned for n in decl) and 'merkle_set' not in pinned
    for older in ('fawkes_hip_sparse_merkle.h', 'fawkes_hip_merkle.h'):
        text = open(os.path.join(INCLUDE, older)).read()
        assert '_set' not in text.replace('fawkes_hip_merkle_set.h', ''), older         # (the new header's file name is all they may say of it)
    assert 'fawkes_hip_merkle_set.h' in open(os.path.join(INCLUDE, 'fawkes_hip_sparse_merkle.h')).read()


def test_header_compiles_alone_as_c99():
    prog = ('#include "fawkes_hip_merkle_set.h"\n'
            'int main(void) { int (*f)(fk_ctx *, fk_smt *, const void *, const void *, size_t, void *) = fk_smt_set_dev; (void)f; return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', INCLUDE, '-c', src, '-o', os.path.join(td, 'alone.o')])
    assert MS.MAX_WRITES == S.MAX_WRITES == M.MAX_WRITES == 1 << 28


def test_the_package_exports_the_module():
    assert fk.merkle_set is MS
    assert all(callable(getattr(MS, n)) for n in ('set_sparse', 'set_sparse_dev', 'set_sparse_timed_dev', 'set_dense', 'set_dense_dev', 'set_dense_timed_dev', 'restore'))
    assert all(callable(getattr(S.SparseMerkleTree, n)) for n in ('set', 'set_dev', 'restore'))
    assert 'restore' in S.__doc__ and 'through `update`' not in S.__doc__


def test_a_null_context_is_refused_by_every_entry_and_nothing_is_written():
    lib = MS._lib()
    idx, leaf = np.zeros(1, np.uint64), np.zeros(4, np.uint64)
    root, ms, distinct = np.full(4, MARK, np.uint64), np.full(2, 0.5), np.full(64, MARK, np.uint64)
    assert lib.fk_smt_set_dev(None, None, None, None, 1, None) == FK_ERR_BAD_ARG
    assert lib.fk_smt_set(None, None, idx.ctypes.data, leaf.ctypes.data, 1, root.ctypes.data) == FK_ERR_BAD_ARG
    assert lib.fk_smt_set_timed_dev(None, None, None, None, 1, None, ms.ctypes.data, distinct.ctypes.data) == FK_ERR_BAD_ARG
    assert lib.fk_poseidon_merkle_set_dev(None, None, None, 3, None, None, 1) == FK_ERR_BAD_ARG
    assert lib.fk_poseidon_merkle_set(None, None, None, 3, idx.ctypes.data, leaf.ctypes.data, 1) == FK_ERR_BAD_ARG
    assert lib.fk_poseidon_merkle_set_timed_dev(None, None, None, 3, None, None, 1, ms.ctypes.data, distinct.ctypes.data) == FK_ERR_BAD_ARG
    assert (root == MARK).all() and (distinct == MARK).all() and (ms == 0.5).all()
