"""
Merkle state on the device (include/fawkes_hip_merkle.h, csrc/merkle_update.hip): ordered leaf writes to a resident Poseidon tree, each
with its proof as of its own moment.

A rollup batch chains -- the old root of transaction j + 1 is the new root of transaction j, and the sibling path of transaction j is the
path in the tree as transactions 0 .. j - 1 left it.  `update` applies k leaf writes IN ORDER to a `MerkleTree` (Context.merkle_tree) and
returns what each transaction's circuit needs: the leaf it replaced, its siblings, the root after it.  One launch of k hashes per level,
whatever the collisions among the indices.

The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
Limits: one GPU; the tree resident and dense (2^(depth + 1) - 1 nodes: for a tree too deep for that, sparse_merkle.SparseMerkleTree
offers the same update over the stored nodes alone); at most 2^28 writes per call.
"""
import ctypes as C

import numpy as np

from . import api
from .api import _fr_ints, _fr_rows, _is_limbs, _vp

MAX_WRITES = 1 << 28

I, U32, P, Z = C.c_int, C.c_uint32, C.c_void_p, C.c_size_t

# one prototype per function of include/fawkes_hip_merkle.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_poseidon_merkle_update_dev': (I, (P, P, P, U32, P, P, Z, P, P, P)),
    'fk_poseidon_merkle_update': (I, (P, P, P, U32, P, P, Z, P, P, P)),
    'fk_poseidon_merkle_update_timed_dev': (I, (P, P, P, U32, P, P, Z, P, P, P, P)),
}

_APPLIED = None


def _lib():
    """the loaded library with this module's prototypes applied (once)"""
    global _APPLIED
    lib = api.load_library()
    if _APPLIED is not lib:
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        _APPLIED = lib
    return lib


class MerkleUpdates:
    """What `update` returns for k writes to a tree of depth d.  root_before: the root the first write started from; old_leaves[j]: the
    leaf write j replaced; siblings[j]: its d siblings at that moment, leaf level first; roots[j]: the root after it (the root before
    write j > 0 is roots[j - 1]).  Canonical ints (siblings a list of k lists) where the leaves were given as ints; Montgomery limb
    arrays of shape (4,), (k, 4), (k, d, 4), (k, 4) where they were given as limbs."""

    def __init__(self, root_before, old_leaves, siblings, roots):
        self.root_before, self.old_leaves, self.siblings, self.roots = root_before, old_leaves, siblings, roots

    @classmethod
    def from_limbs(cls, root_before, old_leaves, siblings, roots, as_limbs):
        """from the four limb arrays of a call: kept as they are, or as canonical ints"""
        if as_limbs:
            return cls(root_before, old_leaves, siblings, roots)
        return cls(_fr_ints(root_before)[0], _fr_ints(old_leaves), _sibling_lists(siblings), _fr_ints(roots))

    def roots_before(self):
        """the root each write started from: [root_before] + roots[:-1]"""
        if isinstance(self.roots, np.ndarray):
            return np.concatenate([self.root_before.reshape(1, 4), self.roots[:-1]])
        return [self.root_before] + list(self.roots[:-1])

    def __len__(self):
        return len(self.roots)

    def __repr__(self):
        return 'MerkleUpdates(%d writes)' % len(self)


def _writes(indices, leaves):
    """the arguments of k writes -> (indices (k,) uint64, leaves (k, 4) Montgomery limbs, k, whether the leaves were given as limbs)"""
    as_limbs = _is_limbs(leaves)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    k = idx.shape[0]
    return idx, _fr_rows(leaves, k), k, as_limbs


def _sibling_lists(sib):
    """(n, depth, 4) limbs -> n lists of depth canonical ints"""
    return [_fr_ints(rows) for rows in sib]


def update_dev(ctx, params, d_nodes, depth, d_indices, d_leaves, k, d_old, d_sib, d_roots):
    """fk_poseidon_merkle_update_dev: everything in device memory; any of d_old, d_sib, d_roots may be None.  Queued on the context's
    stream (ctx.sync() before the outputs are read through another stream)."""
    ctx._ck(_lib().fk_poseidon_merkle_update_dev(ctx.handle, params.handle, d_nodes, depth, d_indices, d_leaves, k, d_old, d_sib, d_roots))


def update_timed_dev(ctx, params, d_nodes, depth, d_indices, d_leaves, k, d_old, d_sib, d_roots):
    """fk_poseidon_merkle_update_timed_dev: update_dev, then a wait -> (ms of the whole update on the device, ms of its hash launches)"""
    ms = (C.c_double * 2)()
    ctx._ck(_lib().fk_poseidon_merkle_update_timed_dev(ctx.handle, params.handle, d_nodes, depth, d_indices, d_leaves, k, d_old, d_sib, d_roots, ms))
    return ms[0], ms[1]


def update(tree, params, indices, leaves):
    """Applies leaves[j] to leaf indices[j] of `tree` (a MerkleTree) for j = 0, 1, ... in this order -> MerkleUpdates.  An index at or
    above tree.n_leaves (below 2^depth) writes into the zero padding: the leaf is appended and tree.n_leaves grows.  leaves: canonical
    ints or an (k, 4) uint64 array of Montgomery limbs.  A refused call (FkError: an index not below 2^depth, t != 3) leaves the tree
    as it was."""
    ctx, depth = tree.ctx, tree.depth
    idx, la, k, as_limbs = _writes(indices, leaves)
    root = ctx.download(tree.d_nodes + 32 * (tree.n_nodes - 1), 32, np.uint64)
    old, sib, roots = np.zeros((k, 4), np.uint64), np.zeros((k, depth, 4), np.uint64), np.zeros((k, 4), np.uint64)
    ctx._ck(_lib().fk_poseidon_merkle_update(ctx.handle, params.handle, tree.d_nodes, depth, _vp(idx), _vp(la), k, _vp(old), _vp(sib) if depth else None, _vp(roots)))
    if k:
        tree._root = None
        tree.n_leaves = max(tree.n_leaves, int(idx.max()) + 1)
    return MerkleUpdates.from_limbs(root, old, sib, roots, as_limbs)
