"""
Bulk leaf writes to the Merkle trees on the device (include/fawkes_hip_merkle_set.h, csrc/merkle_plan.hpp): the final state of an ordered
update, one hash per touched node.

`sparse_merkle.SparseMerkleTree.update` and `merkle.update` apply k writes IN ORDER and return a proof per write: k x depth hashes, what
a rollup batch needs.  `set_sparse` / `set_dense` take the same (indices, leaves), leave the tree in exactly the state that update
leaves it in (for an index given several times the last one wins; a sparse tree stores the same nodes) and return the new root alone,
hashing every distinct touched node once -- for leaves 0 .. k - 1 of a depth-32 tree that is 32 times fewer hashes.  Use them to load a
tree (`restore`), to apply a genesis allocation, to follow a chain's state; use `update` where the proofs are wanted.

The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
Limits: one GPU; at most 2^28 writes per call.
"""
import ctypes as C

import numpy as np

from . import api
from .api import _fr_ints, _vp
from .merkle import _writes

MAX_WRITES = 1 << 28

I, U32, P, Z = C.c_int, C.c_uint32, C.c_void_p, C.c_size_t

# one prototype per function of include/fawkes_hip_merkle_set.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_smt_set_dev': (I, (P, P, P, P, Z, P)),
    'fk_smt_set': (I, (P, P, P, P, Z, P)),
    'fk_smt_set_timed_dev': (I, (P, P, P, P, Z, P, P, P)),
    'fk_poseidon_merkle_set_dev': (I, (P, P, P, U32, P, P, Z)),
    'fk_poseidon_merkle_set': (I, (P, P, P, U32, P, P, Z)),
    'fk_poseidon_merkle_set_timed_dev': (I, (P, P, P, U32, P, P, Z, P, P)),
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


# ---- sparse trees
def set_sparse_dev(tree, d_indices, d_leaves, k, d_root=None):
    """fk_smt_set_dev: everything in device memory; d_root (one Fr) may be None.  Queued on the context's stream"""
    tree.ctx._ck(_lib().fk_smt_set_dev(tree.ctx.handle, tree.handle, d_indices, d_leaves, k, d_root))


def set_sparse_timed_dev(tree, d_indices, d_leaves, k, d_root=None):
    """fk_smt_set_timed_dev: set_sparse_dev, then a wait -> (ms of the whole call on the device, ms of its hash launches, distinct):
    distinct[l], l = 0 .. depth, the number of distinct touched nodes of level l -- what was stored and hashed there ([] for k = 0)"""
    ms = (C.c_double * 2)()
    distinct = np.zeros(tree.depth + 1, np.uint64)
    tree.ctx._ck(_lib().fk_smt_set_timed_dev(tree.ctx.handle, tree.handle, d_indices, d_leaves, k, d_root, ms, _vp(distinct)))
    return ms[0], ms[1], [int(x) for x in distinct] if k else []


def set_sparse(tree, indices, leaves):
    """Leaves `tree` (a SparseMerkleTree) as `tree.update(indices, leaves)` leaves it -> the new root (a canonical int where the leaves
    were ints, 4 limbs where they were an (k, 4) uint64 array).  A refused call (FkError: an index not below 2^depth) leaves the tree as
    it was."""
    ctx = tree.ctx
    idx, la, k, as_limbs = _writes(indices, leaves)
    root = np.zeros(4, np.uint64)
    ctx._ck(_lib().fk_smt_set(ctx.handle, tree.handle, _vp(idx), _vp(la), k, _vp(root)))
    if not k:
        root = tree.root_limbs()
    return root if as_limbs else _fr_ints(root)[0]


def restore(ctx, params, depth, indices, leaves, expected_leaves=0):
    """-> a new SparseMerkleTree given its leaves by one `set_sparse`: restore(ctx, params, old.depth, *old.leaves()) has old's root and
    stores what old stores.  expected_leaves: as in SparseMerkleTree (0: the smallest tables, grown by the set as it needs)"""
    from .sparse_merkle import SparseMerkleTree
    tree = SparseMerkleTree(ctx, params, depth, expected_leaves)
    try:
        set_sparse(tree, indices, leaves)
    except Exception:
        tree.free()
        raise
    return tree


# ---- dense trees
def set_dense_dev(ctx, params, d_nodes, depth, d_indices, d_leaves, k):
    """fk_poseidon_merkle_set_dev: everything in device memory.  Queued on the context's stream"""
    ctx._ck(_lib().fk_poseidon_merkle_set_dev(ctx.handle, params.handle, d_nodes, depth, d_indices, d_leaves, k))


def set_dense_timed_dev(ctx, params, d_nodes, depth, d_indices, d_leaves, k):
    """fk_poseidon_merkle_set_timed_dev: set_dense_dev, then a wait -> (ms, ms of the hash launches, distinct) as set_sparse_timed_dev"""
    ms = (C.c_double * 2)()
    distinct = np.zeros(depth + 1, np.uint64)
    ctx._ck(_lib().fk_poseidon_merkle_set_timed_dev(ctx.handle, params.handle, d_nodes, depth, d_indices, d_leaves, k, ms, _vp(distinct)))
    return ms[0], ms[1], [int(x) for x in distinct] if k else []


def set_dense(tree, params, indices, leaves):
    """Leaves `tree` (a MerkleTree) as `merkle.update(tree, params, indices, leaves)` leaves it -> the new root (int or limbs, as the
    leaves were given).  An index at or above tree.n_leaves appends, as there.  A refused call (FkError: an index not below 2^depth,
    t != 3) leaves the tree as it was."""
    ctx, depth = tree.ctx, tree.depth
    idx, la, k, as_limbs = _writes(indices, leaves)
    ctx._ck(_lib().fk_poseidon_merkle_set(ctx.handle, params.handle, tree.d_nodes, depth, _vp(idx), _vp(la), k))
    if k:
        tree._root = None
        tree.n_leaves = max(tree.n_leaves, int(idx.max()) + 1)
    root = ctx.download(tree.d_nodes + 32 * (tree.n_nodes - 1), 32, np.uint64)
    return root if as_limbs else _fr_ints(root)[0]
