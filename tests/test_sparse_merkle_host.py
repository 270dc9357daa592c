"""The sparse Merkle tree without a GPU: include/fawkes_hip_sparse_merkle.h against the library and the ctypes table of
fawkes_crypto_amd/sparse_merkle.py, the package export, the refusals that need no device, and the tests' own reference
(tests/sparse_merkle_cases.py: the in-order walk over dicts) against the dense walk of tests/merkle_cases.py."""
import os
import re
import subprocess
import tempfile

import numpy as np

import fawkes_crypto_amd as fk
from fawkes_crypto_amd import merkle as M
from fawkes_crypto_amd import sparse_merkle as S
import merkle_cases as mc
import sparse_merkle_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'fawkes_hip_sparse_merkle.h')
FK_ERR_BAD_ARG = 1


def _declared():
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b(fk_\w+)\s*\(([^()]*)\)\s*;', text):
        out[name] = len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])
    return out


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(S.PROTOTYPES) and len(decl) == 11
    assert decl['fk_smt_update_dev'] == decl['fk_smt_update'] == 8 and decl['fk_smt_update_timed_dev'] == 9
    assert decl['fk_smt_proofs_dev'] == decl['fk_smt_proofs'] == 6 and decl['fk_smt_new'] == 5 and decl['fk_smt_export_level'] == 7
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(S.PROTOTYPES[name][1]) == nargs, name
    # kept out of the pinned ABI, and out of the dense header
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    assert 'fk_smt' not in open(os.path.join(ROOT, 'include', 'fawkes_hip.h')).read()
    assert not set(decl) & set(M.PROTOTYPES)


def test_header_compiles_alone_as_c99_and_the_constants_have_their_values():
    prog = ('#include "fawkes_hip_sparse_merkle.h"\n'
            'int main(void) { fk_smt *t = 0; (void)t; return FK_SMT_MAX_DEPTH == 63 && FK_SMT_MIN_SLOTS == 64 && FK_SMT_MAX_WRITES == 268435456u ? 0 : 1; }\n')
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])
    assert (S.MAX_DEPTH, S.MIN_SLOTS, S.MAX_WRITES) == (63, 64, 1 << 28)


def test_the_package_exports_the_module():
    assert fk.sparse_merkle is S and fk.SparseMerkleTree is S.SparseMerkleTree
    assert all(callable(getattr(S.SparseMerkleTree, n)) for n in ('update', 'update_dev', 'update_timed_dev', 'proofs', 'proofs_dev', 'level', 'leaves', 'info', 'free'))
    assert isinstance(S.SparseMerkleTree.root, property) and isinstance(S.SparseMerkleTree.defaults, property)
    assert 'sparse_merkle' in M.__doc__


def test_refusals_that_need_no_device():
    """a null context is refused by every entry before anything is looked at, and so is a null tree where no context is asked for"""
    lib = S._lib()
    idx, leaf, out = np.zeros(1, np.uint64), np.zeros(4, np.uint64), np.zeros(8, np.uint64)
    n = S.C.c_size_t(7)
    h = S.C.c_void_p()
    assert lib.fk_smt_new(None, None, 3, 0, S.C.byref(h)) == FK_ERR_BAD_ARG and not h.value
    assert lib.fk_smt_info(None, None, out.ctypes.data) == FK_ERR_BAD_ARG
    assert lib.fk_smt_root(None, None, out.ctypes.data) == FK_ERR_BAD_ARG
    assert lib.fk_smt_defaults(None, out.ctypes.data) == FK_ERR_BAD_ARG
    assert lib.fk_smt_update_dev(None, None, None, None, 1, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_smt_update(None, None, idx.ctypes.data, leaf.ctypes.data, 1, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_smt_update_timed_dev(None, None, None, None, 1, None, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_smt_proofs_dev(None, None, None, 1, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_smt_proofs(None, None, idx.ctypes.data, 1, out.ctypes.data, None) == FK_ERR_BAD_ARG
    assert lib.fk_smt_export_level(None, None, 0, None, None, 0, S.C.byref(n)) == FK_ERR_BAD_ARG and n.value == 7
    lib.fk_smt_free(None, None)          # nothing to free: returns
    assert not out.any()


def _assert_equals_the_dense_walk(c):
    s = sc.from_dense(c)
    assert s.root_before == c.root_before
    assert (s.old, s.siblings, s.roots) == (c.old, c.siblings, c.roots)
    # every stored node is the dense final tree's, and every dense node that is not its level's default is stored
    off = 0
    for l in range(c.depth + 1):
        dense = c.nodes[off:off + (1 << (c.depth - l))]
        off += len(dense)
        assert all(dense[i] == v for i, v in s.levels[l].items())
        assert all(i in s.levels[l] for i, v in enumerate(dense) if v != s.tree.zero[l])
    assert s.tree.root == c.nodes[-1]


def test_the_sparse_walk_equals_the_dense_walk():
    _assert_equals_the_dense_walk(mc.case('hot', 65))
    _assert_equals_the_dense_walk(mc.case('edges'))


def test_the_defaults_are_the_roots_of_zero_trees():
    z = sc.defaults(5)
    assert z[0] == 0
    for d in range(6):
        assert z[d] == mc.build_levels([0], d)[d][0], d
    w = sc.SparseWalk(4)
    assert w.root == z[4] and w.proof(9) == (0, z[:4])
