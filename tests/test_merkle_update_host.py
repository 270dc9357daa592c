"""The Merkle update without a GPU: include/fawkes_hip_merkle.h against the library and the ctypes table of fawkes_crypto_amd/merkle.py,
the package export, the refusals that need no device, and the tests' own reference (tests/merkle_cases.py: the in-order walk) against a
rebuild and against the oracle's proof roots."""
import os
import re
import subprocess
import tempfile

import numpy as np

import fawkes_crypto_amd as fk
from fawkes_crypto_amd import merkle as M
import merkle_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'fawkes_hip_merkle.h')
FK_ERR_BAD_ARG = 1


def _declared():
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b(fk_\w+)\s*\(([^()]*)\)\s*;', text):
        out[name] = len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])
    return out


def test_the_library_exports_both_entry_points():
    lib = fk.load_library()
    assert hasattr(lib, 'fk_poseidon_merkle_update_dev') and hasattr(lib, 'fk_poseidon_merkle_update')


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(M.PROTOTYPES) and len(decl) == 3
    assert decl['fk_poseidon_merkle_update_dev'] == decl['fk_poseidon_merkle_update'] == 10
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(M.PROTOTYPES[name][1]) == nargs, name
    # kept out of the pinned ABI
    assert not any(n in fk.EXPORTED_SYMBOLS for n in decl)
    assert 'merkle_update' not in open(os.path.join(ROOT, 'include', 'fawkes_hip.h')).read()


def test_header_compiles_alone_as_c99():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include "fawkes_hip_merkle.h"\nint main(void) { return FK_MERKLE_UPDATE_MAX_WRITES == 268435456u ? 0 : 1; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])
    assert M.MAX_WRITES == 1 << 28


def test_the_package_exports_the_module():
    assert fk.merkle is M
    assert callable(M.update) and callable(M.update_dev) and M.MerkleUpdates.__name__ == 'MerkleUpdates'


def test_refusals_that_need_no_device():
    """a null context is refused by every entry before anything is looked at"""
    lib = M._lib()
    idx, leaf = np.zeros(1, np.uint64), np.zeros(4, np.uint64)
    assert lib.fk_poseidon_merkle_update_dev(None, None, None, 0, None, None, 1, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_poseidon_merkle_update(None, None, None, 0, idx.ctypes.data, leaf.ctypes.data, 1, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_poseidon_merkle_update_timed_dev(None, None, None, 0, None, None, 1, None, None, None, None) == FK_ERR_BAD_ARG


def test_the_reference_walk_is_consistent():
    mc.self_check()
    c = mc.case('depth1_10')
    assert c.siblings[0] == [c.leaves[0]] and c.siblings[1] == [c.values[0]] and c.old == [c.leaves[1], c.leaves[0]]
    c = mc.case('alternate')
    assert all(c.siblings[j][0] == c.values[j - 1] for j in range(1, 64))
    c = mc.case('edges')
    assert c.n_leaves == 8 and c.old[2] == 0 and c.old[5] == c.values[2]
