"""
Sparse Merkle state on the device (include/fawkes_hip_sparse_merkle.h, csrc/sparse_merkle.hip): a Poseidon tree of depth up to 63 of
which only the nodes ever written are stored -- the account tree of a rollup (depth 32) beside a proving key.

An untouched subtree at level l has the value defaults[l] (defaults[0] = 0, defaults[l + 1] = H(defaults[l], defaults[l])): what a
dense tree gives its zero padding, so a `SparseMerkleTree` and a `MerkleTree` over the same leaves agree on every root and sibling.
`update` is `merkle.update`'s contract (k leaf writes IN ORDER -> merkle.MerkleUpdates); `proofs` reads without changing anything;
`leaves()` is how a tree is saved: `SparseMerkleTree.restore(ctx, params, depth, *tree.leaves())` is a new tree with the same root and
the same stored nodes (merkle_set.py: one bulk write, one hash per node).  `set` is that bulk write on its own: the final state of
`update`, the new root and no proofs.

The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
Limits: one GPU; at most 2^28 writes per call; entries are never removed (a leaf written back to 0 stays stored).
"""
import ctypes as C

import numpy as np

from . import api
from .api import _fr_ints, _vp
from .merkle import MerkleUpdates, _sibling_lists, _writes

MAX_DEPTH = 63
MIN_SLOTS = 64
MAX_WRITES = 1 << 28

I, U32, U64, P, Z = C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t

# one prototype per function of include/fawkes_hip_sparse_merkle.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_smt_new': (I, (P, P, U32, U64, P)),
    'fk_smt_free': (None, (P, P)),
    'fk_smt_info': (I, (P, P, P)),
    'fk_smt_defaults': (I, (P, P)),
    'fk_smt_root': (I, (P, P, P)),
    'fk_smt_update_dev': (I, (P, P, P, P, Z, P, P, P)),
    'fk_smt_update': (I, (P, P, P, P, Z, P, P, P)),
    'fk_smt_update_timed_dev': (I, (P, P, P, P, Z, P, P, P, P)),
    'fk_smt_proofs_dev': (I, (P, P, P, Z, P, P)),
    'fk_smt_proofs': (I, (P, P, P, Z, P, P)),
    'fk_smt_export_level': (I, (P, P, U32, P, P, Z, P)),
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


class SparseMerkleTree(api._Handle):
    """An empty tree of 2^depth zero leaves in the device memory of `ctx`, hashing with `params` (t = 3; the tree keeps its own copy).
    expected_leaves sizes the tables so that this many distinct leaves fit without a growth (0: the smallest tables, grown as needed).
    Free it before its context."""

    def __init__(self, ctx, params, depth, expected_leaves=0):
        self.ctx, self.depth = ctx, int(depth)
        if not 0 <= self.depth < 1 << 32 or not 0 <= int(expected_leaves) < 1 << 64:
            raise api.FkError(1, 'sparse merkle: depth and expected_leaves must be non-negative integers')
        h = C.c_void_p()
        ctx._ck(_lib().fk_smt_new(ctx.handle, params.handle, self.depth, int(expected_leaves), C.byref(h)))
        self.handle = h

    def _release(self, h):
        if self.ctx.handle:
            _lib().fk_smt_free(self.ctx.handle, h)

    # ---- reading
    def root_limbs(self):
        out = np.zeros(4, np.uint64)
        self.ctx._ck(_lib().fk_smt_root(self.ctx.handle, self.handle, _vp(out)))
        return out

    @property
    def root(self):
        return _fr_ints(self.root_limbs())[0]

    @property
    def defaults(self):
        """defaults[l], l = 0 .. depth: the value of an untouched subtree at level l (canonical ints); defaults[depth] is the empty root"""
        out = np.zeros((self.depth + 1, 4), np.uint64)
        api._check(_lib().fk_smt_defaults(self.handle, _vp(out)), 'fk_smt_defaults')
        return _fr_ints(out)

    def info(self):
        """dict(depth, leaves, nodes, device_bytes): stored leaves, stored nodes of all levels, bytes of device memory"""
        out = np.zeros(4, np.uint64)
        self.ctx._ck(_lib().fk_smt_info(self.ctx.handle, self.handle, _vp(out)))
        return dict(depth=int(out[0]), leaves=int(out[1]), nodes=int(out[2]), device_bytes=int(out[3]))

    def level_limbs(self, l):
        """the stored entries of level l ascending by key -> (keys (n,) uint64, values (n, 4) Montgomery limbs)"""
        lib, n = _lib(), C.c_size_t()
        self.ctx._ck(lib.fk_smt_export_level(self.ctx.handle, self.handle, l, None, None, 0, C.byref(n)))
        keys, vals = np.zeros(n.value, np.uint64), np.zeros((n.value, 4), np.uint64)
        if n.value:
            self.ctx._ck(lib.fk_smt_export_level(self.ctx.handle, self.handle, l, _vp(keys), _vp(vals), n.value, C.byref(n)))
        return keys, vals

    def level(self, l):
        """{node index: value} of the stored entries of level l (0 = leaves .. depth = the root alone), canonical ints, ascending"""
        keys, vals = self.level_limbs(l)
        return dict(zip((int(x) for x in keys), _fr_ints(vals)))

    def leaves(self):
        """(indices, values) of the stored leaves ascending by index: given to `restore` they make a new tree with the same root"""
        lv = self.level(0)
        return list(lv), list(lv.values())

    def proofs_dev(self, d_indices, n, d_leaves, d_siblings):
        """fk_smt_proofs_dev: everything in device memory; either output may be None.  Changes nothing"""
        self.ctx._ck(_lib().fk_smt_proofs_dev(self.ctx.handle, self.handle, d_indices, n, d_leaves, d_siblings))

    def proofs(self, indices, as_limbs=False):
        """-> (leaves, siblings) of the given leaf indices, written or not: leaves[i] (0 where none was written), siblings[i] = its depth
        siblings, leaf level first (defaults[l] where the subtree is untouched).  Canonical ints, or limb arrays (n, 4), (n, depth, 4)"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        n, depth = idx.shape[0], self.depth
        lv, sib = np.zeros((n, 4), np.uint64), np.zeros((n, depth, 4), np.uint64)
        self.ctx._ck(_lib().fk_smt_proofs(self.ctx.handle, self.handle, _vp(idx), n, _vp(lv), _vp(sib) if depth else None))
        return (lv, sib) if as_limbs else (_fr_ints(lv), _sibling_lists(sib))

    # ---- writing
    def update_dev(self, d_indices, d_leaves, k, d_old, d_sib, d_roots):
        """fk_smt_update_dev: everything in device memory; any of d_old, d_sib, d_roots may be None.  Queued on the context's stream"""
        self.ctx._ck(_lib().fk_smt_update_dev(self.ctx.handle, self.handle, d_indices, d_leaves, k, d_old, d_sib, d_roots))

    def update_timed_dev(self, d_indices, d_leaves, k, d_old, d_sib, d_roots):
        """fk_smt_update_timed_dev: update_dev, then a wait -> (ms of the whole update on the device, ms of its hash launches)"""
        ms = (C.c_double * 2)()
        self.ctx._ck(_lib().fk_smt_update_timed_dev(self.ctx.handle, self.handle, d_indices, d_leaves, k, d_old, d_sib, d_roots, ms))
        return ms[0], ms[1]

    def update(self, indices, leaves):
        """Applies leaves[j] to leaf indices[j] for j = 0, 1, ... in this order -> merkle.MerkleUpdates (canonical ints where the leaves
        were ints, limb arrays where they were an (k, 4) uint64 array).  A refused call (FkError: an index not below 2^depth) leaves
        the tree as it was."""
        ctx, depth = self.ctx, self.depth
        idx, la, k, as_limbs = _writes(indices, leaves)
        root = self.root_limbs()
        old, sib, roots = np.zeros((k, 4), np.uint64), np.zeros((k, depth, 4), np.uint64), np.zeros((k, 4), np.uint64)
        ctx._ck(_lib().fk_smt_update(ctx.handle, self.handle, _vp(idx), _vp(la), k, _vp(old), _vp(sib) if depth else None, _vp(roots)))
        return MerkleUpdates.from_limbs(root, old, sib, roots, as_limbs)

    # ---- bulk writes (merkle_set.py, imported where it is used: that module imports this one's class)
    def set(self, indices, leaves):
        """merkle_set.set_sparse: the final state of `update(indices, leaves)`, one hash per touched node -> the new root"""
        from . import merkle_set
        return merkle_set.set_sparse(self, indices, leaves)

    def set_dev(self, d_indices, d_leaves, k, d_root=None):
        """merkle_set.set_sparse_dev: everything in device memory; d_root may be None"""
        from . import merkle_set
        merkle_set.set_sparse_dev(self, d_indices, d_leaves, k, d_root)

    @classmethod
    def restore(cls, ctx, params, depth, indices, leaves, expected_leaves=0):
        """merkle_set.restore: a new tree given its leaves by one `set`"""
        from . import merkle_set
        return merkle_set.restore(ctx, params, depth, indices, leaves, expected_leaves)
