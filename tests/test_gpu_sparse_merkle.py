"""The sparse Poseidon Merkle tree on the device (csrc/sparse_merkle.hip through fawkes_crypto_amd/sparse_merkle.py): empty trees and
their defaults; every case of tests/merkle_cases.py against the dense walk, stored nodes included; depth 32 and depth 63 against the
sparse walk (tests/sparse_merkle_cases.py); growth of the tables, byte for byte against the dense update; device-only consistency at a
size the oracle cannot reach; NULL outputs, refusals, the empty call; read-only proofs; the chained batch; the claim on the staging
buffers.  Every comparison is exact equality of canonical integers or bytes."""
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import fawkes_circuit as fc
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import merkle as M
from fawkes_crypto_amd import sparse_merkle as S
import merkle_cases as mc
import sparse_merkle_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0xa5a5a5a5a5a5a5a5
OUTPUTS = ('old', 'sib', 'roots')
ints = fk.api._fr_ints
rows = fk.api._fr_rows


@pytest.fixture(scope='module')
def p3():
    return fk.PoseidonParams(3, 8, 53)


class DevArgs:
    """k writes in device memory, and marked output arrays"""

    def __init__(self, ctx, depth, indices, leaves_mont):
        self.ctx, self.k, self.depth = ctx, len(indices), depth
        k = self.k
        self.sizes = dict(idx=8 * k, new=32 * k, old=32 * k, sib=32 * k * depth, roots=32 * k)
        self.d = {n: ctx.dev_alloc(max(b, 32)) for n, b in self.sizes.items()}
        if k:
            ctx.upload(self.d['idx'], np.asarray(indices, np.uint64))
            ctx.upload(self.d['new'], leaves_mont)
        for n in OUTPUTS:
            if self.sizes[n]:
                ctx.upload(self.d[n], np.full(self.sizes[n] // 8, MARK, np.uint64))

    def get(self, name):
        return self.ctx.download(self.d[name], self.sizes[name], np.uint64).reshape(-1, 4) if self.sizes[name] else np.zeros((0, 4), np.uint64)

    def marked(self, name):
        return bool((self.get(name) == MARK).all())

    def free(self):
        for p in self.d.values():
            self.ctx.dev_free(p)


def run_dev(ctx, tree, indices, values, outputs=OUTPUTS, sync=True):
    """fk_smt_update_dev with the named outputs (the others NULL) -> DevArgs (the caller frees)"""
    a = DevArgs(ctx, tree.depth, indices, rows(values, len(indices)))
    try:
        tree.update_dev(a.d['idx'], a.d['new'], a.k, *(a.d[n] if n in outputs else None for n in OUTPUTS))
        if sync:
            ctx.sync()
    except Exception:
        a.free()
        raise
    return a


def populate(ctx, tree, pairs):
    """the initial leaves: a first update with all outputs NULL"""
    if pairs:
        run_dev(ctx, tree, [i for i, _ in pairs], [v for _, v in pairs], ()).free()


def dense_levels(c):
    out, off = [], 0
    for l in range(c.depth + 1):
        out.append(c.nodes[off:off + (1 << (c.depth - l))])
        off += len(out[-1])
    return out


def assert_stored_is_dense(tree, c):
    """every stored entry of every level equals the dense final tree's node; every dense node that differs from zero[l] is stored"""
    zero = tree.defaults
    for l, dense in enumerate(dense_levels(c)):
        stored = tree.level(l)
        assert list(stored) == sorted(stored)
        assert all(dense[i] == v for i, v in stored.items()), l
        assert all(i in stored for i, v in enumerate(dense) if v != zero[l]), l
    assert tree.root == c.nodes[-1]


def assert_levels(tree, levels):
    for l in range(tree.depth + 1):
        assert tree.level(l) == dict(sorted(levels[l].items())), l


def sparse_from_dense_case(ctx, p3, c):
    tree = S.SparseMerkleTree(ctx, p3, c.depth)
    populate(ctx, tree, list(enumerate(c.leaves)))
    return tree


# ---------------------------------------------------------------- empty trees
@pytest.mark.parametrize('depth', [0, 1, 5, 32, 63])
def test_an_empty_tree_has_the_default_root(ctx, p3, depth):
    tree = S.SparseMerkleTree(ctx, p3, depth)
    want = sc.defaults(depth)
    assert tree.defaults == want and tree.root == want[depth]
    info = tree.info()
    assert info['depth'] == depth and info['nodes'] == 0 and info['leaves'] == (0 if depth else 1)
    assert info['device_bytes'] >= depth * S.MIN_SLOTS * 40
    assert all(tree.level(l) == {} for l in range(depth)) and tree.level(depth) == {0: want[depth]}
    tree.free()


# ---------------------------------------------------------------- against the dense walk on the oracle
CASES = [('depth0', 0), ('depth1_01', 0), ('depth1_10', 0), ('one_index', 0), ('alternate', 0), ('edges', 0)] + [('hot', k) for k in (1, 63, 64, 65, 257)]


@pytest.mark.parametrize('name,k', CASES)
def test_every_dense_case_equals_the_walk(ctx, p3, name, k):
    c = mc.case(name, k)
    tree = sparse_from_dense_case(ctx, p3, c)
    upd = tree.update(c.indices, c.values)
    assert upd.root_before == c.root_before
    assert upd.old_leaves == c.old
    assert upd.siblings == c.siblings
    assert upd.roots == c.roots
    assert_stored_is_dense(tree, c)
    tree.free()


@pytest.mark.parametrize('k', [1, 65, 257])
def test_hot_set_device_arrays_equal_the_walk(ctx, p3, k):
    c = mc.case('hot', k)
    tree = sparse_from_dense_case(ctx, p3, c)
    a = run_dev(ctx, tree, c.indices, c.values)
    try:
        assert ints(a.get('old')) == c.old
        assert ints(a.get('sib')) == [s for row in c.siblings for s in row]
        assert ints(a.get('roots')) == c.roots
        assert_stored_is_dense(tree, c)
    finally:
        a.free()
        tree.free()


# ---------------------------------------------------------------- deep trees against the sparse walk
@pytest.mark.parametrize('name', ['deep32', 'deep63'])
def test_deep_cases_equal_the_sparse_walk(ctx, p3, name):
    c = sc.case(name)
    if name == 'deep32':
        assert len(c.indices) == 40 and {0, (1 << 32) - 1} <= set(c.indices) and max(c.indices.count(i) for i in c.indices) == 3
    else:
        assert len(c.indices) == 16 and (1 << 63) - 1 in c.indices and sum(i >= 1 << 62 for i in c.indices) >= 5
    tree = S.SparseMerkleTree(ctx, p3, c.depth)
    populate(ctx, tree, c.initial)
    upd = tree.update(c.indices, c.values)
    assert upd.root_before == c.root_before
    assert (upd.old_leaves, upd.siblings, upd.roots) == (c.old, c.siblings, c.roots)
    assert_levels(tree, c.levels)
    info = tree.info()
    assert info['leaves'] == len(c.levels[0]) and info['nodes'] == sum(len(lv) for lv in c.levels[:c.depth])
    # read-only proofs, of written leaves and of leaves never written: the stored value or the level's default
    never = [i for i in (1, 0x12345670, (1 << c.depth) - 3, 1 << (c.depth - 1)) if i not in c.levels[0]]
    ask = never + c.indices[:4]
    leaves, sibs = tree.proofs(ask)
    assert (leaves, sibs) == ([c.tree.proof(i)[0] for i in ask], [c.tree.proof(i)[1] for i in ask])
    assert leaves[:len(never)] == [0] * len(never) and len(never) >= 2
    zero = tree.defaults
    assert any(s == zero[l] for row in sibs[:len(never)] for l, s in enumerate(row)) and any(s != zero[l] for row in sibs[:len(never)] for l, s in enumerate(row))
    assert tree.info() == info and tree.root == c.roots[-1]
    tree.free()


# ---------------------------------------------------------------- growth of the tables, against the dense update
def test_growth_gives_what_the_dense_update_gives(ctx, p3):
    depth, per = 12, 300
    rnd = random.Random(12)
    all_idx = rnd.sample(range(1 << depth), 3 * per)
    dense = ctx.merkle_tree(p3, np.zeros((1 << depth, 4), np.uint64))
    tree = S.SparseMerkleTree(ctx, p3, depth, 0)
    queued = S.SparseMerkleTree(ctx, p3, depth, 0)         # the same writes through update_dev, nothing waited for in between
    assert per > S.MIN_SLOTS // 2
    bytes_seen, batches = [tree.info()['device_bytes']], []
    try:
        for r in range(3):
            idx = np.asarray(all_idx[r * per:(r + 1) * per], np.uint64)
            vals = rows([rnd.randrange(1, mc.R) for _ in range(per)])
            want = M.update(dense, p3, idx, vals)
            got = tree.update(idx, vals)
            for name in ('root_before', 'old_leaves', 'siblings', 'roots'):
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (r, name)
            info = tree.info()
            assert info['leaves'] == (r + 1) * per
            bytes_seen.append(info['device_bytes'])
            batches.append(run_dev(ctx, queued, idx, vals, (), sync=False))
        assert bytes_seen[1] > bytes_seen[0] and bytes_seen[2] > bytes_seen[1]          # level 0 grew more than once
        assert queued.root_limbs().tobytes() == tree.root_limbs().tobytes() and queued.info() == tree.info()
        for l in range(depth + 1):
            k1, v1 = tree.level_limbs(l)
            k2, v2 = queued.level_limbs(l)
            assert k1.tobytes() == k2.tobytes() and v1.tobytes() == v2.tobytes(), l
        nodes, off = dense.nodes(), 0
        for l in range(depth):                                                          # what is stored is the dense tree's
            keys, vals = tree.level_limbs(l)
            assert nodes[off + keys.astype(np.int64)].tobytes() == vals.tobytes(), l
            off += 1 << (depth - l)
    finally:
        for a in batches:
            a.free()
        dense.free(); tree.free(); queued.free()


# ---------------------------------------------------------------- device only: 3000 leaves, 5000 writes
@pytest.mark.parametrize('depth', [32, 12])
def test_5000_writes_are_consistent_on_the_device(ctx, p3, depth):
    k, n0 = 5000, 3000
    rnd = random.Random(5000 + depth)
    first = rnd.sample(range(1 << depth), n0)
    hot = rnd.sample(range(1 << depth), 16)
    indices = [rnd.choice(hot) if j & 1 else rnd.randrange(1 << depth) for j in range(k)]
    leaves = rows(mc.values_for(n0, rnd))
    values = rows(mc.values_for(k, rnd))
    tree = S.SparseMerkleTree(ctx, p3, depth, n0)
    run_dev(ctx, tree, first, leaves, ()).free()
    root_before = tree.root_limbs()
    a = run_dev(ctx, tree, indices, values)
    d_out = ctx.dev_alloc(32 * k)
    rebuilt = S.SparseMerkleTree(ctx, p3, depth)
    try:
        roots = a.get('roots')
        ctx.merkle_proof_roots_dev(p3, a.d['old'], a.d['sib'], a.d['idx'], depth, k, d_out)
        got = ctx.download(d_out, 32 * k, np.uint64).reshape(-1, 4)
        assert got.tobytes() == np.concatenate([root_before.reshape(1, 4), roots[:-1]]).tobytes()
        ctx.merkle_proof_roots_dev(p3, a.d['new'], a.d['sib'], a.d['idx'], depth, k, d_out)
        assert ctx.download(d_out, 32 * k, np.uint64).tobytes() == roots.tobytes()
        root = tree.root_limbs()
        assert root.tobytes() == roots[-1].tobytes()
        # the leaf export is the tree: a new tree given it has the same root, and every stored leaf's proof recomputes to the root
        keys, vals = tree.level_limbs(0)
        assert len(keys) == len(set(first) | set(indices)) == tree.info()['leaves'] and (keys[1:] > keys[:-1]).all()
        rebuilt.update(keys, vals)
        assert rebuilt.root_limbs().tobytes() == root.tobytes()
        lv, sib = tree.proofs(keys, as_limbs=True)
        assert lv.tobytes() == vals.tobytes()
        assert ctx.merkle_proof_roots(p3, lv, sib, keys, depth).tobytes() == np.tile(root, (len(keys), 1)).tobytes()
        if depth == 12:                                                                # byte-equal to the dense update's three outputs
            final = np.zeros((1 << depth, 4), np.uint64)
            final[first] = leaves
            dense = ctx.merkle_tree(p3, final)
            try:
                assert dense.nodes()[-1].tobytes() == root_before.tobytes()
                want = M.update(dense, p3, np.asarray(indices, np.uint64), values)
                assert a.get('old').tobytes() == want.old_leaves.tobytes()
                assert a.get('sib').tobytes() == want.siblings.tobytes()
                assert roots.tobytes() == want.roots.tobytes()
            finally:
                dense.free()
    finally:
        ctx.dev_free(d_out)
        a.free()
        tree.free(); rebuilt.free()


def test_2p17_writes_from_512_workgroups_claim_their_slots_consistently(ctx, p3):
    """more workgroups than the device has compute units insert into tables that start at their smallest: the slot claims of one launch
    race across the whole chip, behind a growth of every level.  Every second write goes to a hot set of 4096 leaves"""
    depth, k = 32, 1 << 17
    rng = np.random.default_rng(17)
    hot = rng.integers(0, 1 << depth, 4096, dtype=np.uint64)
    idx = rng.integers(0, 1 << depth, k, dtype=np.uint64)
    idx[1::2] = hot[rng.integers(0, 4096, k // 2)]
    tree, rebuilt = S.SparseMerkleTree(ctx, p3, depth), S.SparseMerkleTree(ctx, p3, depth)
    sizes = dict(idx=8 * k, new=32 * k, old=32 * k, sib=32 * k * depth, roots=32 * k, out=32 * k)
    d = {n: ctx.dev_alloc(b) for n, b in sizes.items()}
    try:
        ctx.upload(d['idx'], idx)
        ctx.gen_scalars_dev(d['new'], k, 17)
        assert tree.root_limbs().tobytes() == fk.api._fr_rows([tree.defaults[depth]])[0].tobytes()
        tree.update_dev(d['idx'], d['new'], k, None, None, None)              # the same writes twice: inserts, then overwrites
        mid = tree.root_limbs()
        tree.update_dev(d['idx'], d['new'], k, d['old'], d['sib'], d['roots'])
        roots = ctx.download(d['roots'], 32 * k, np.uint64).reshape(-1, 4)
        ctx.merkle_proof_roots_dev(p3, d['new'], d['sib'], d['idx'], depth, k, d['out'])
        assert ctx.download(d['out'], 32 * k, np.uint64).tobytes() == roots.tobytes()
        ctx.merkle_proof_roots_dev(p3, d['old'], d['sib'], d['idx'], depth, k, d['out'])
        before = ctx.download(d['out'], 32 * k, np.uint64).reshape(-1, 4)
        assert before[1:].tobytes() == roots[:-1].tobytes() and before[0].tobytes() == mid.tobytes()
        info = tree.info()
        assert info['leaves'] == len(np.unique(idx))
        keys, vals = tree.level_limbs(0)
        assert keys.tobytes() == np.unique(idx).tobytes()
        rebuilt.update(keys, vals)
        assert rebuilt.root_limbs().tobytes() == tree.root_limbs().tobytes() == roots[-1].tobytes()
        assert rebuilt.info()['nodes'] == info['nodes']
    finally:
        for p in d.values():
            ctx.dev_free(p)
        tree.free(); rebuilt.free()


# ---------------------------------------------------------------- NULL outputs, refusals, the empty call
@pytest.mark.parametrize('outputs', [s for n in range(4) for s in itertools.combinations(OUTPUTS, n)])
def test_null_outputs_leave_the_same_tree(ctx, p3, outputs):
    c = mc.case('hot', 65)
    tree = sparse_from_dense_case(ctx, p3, c)
    a = run_dev(ctx, tree, c.indices, c.values, outputs)
    try:
        assert_stored_is_dense(tree, c)
        assert_levels(tree, sc.from_dense(c).levels)
        for n in OUTPUTS:                                                   # what was not asked for was not written
            if n not in outputs:
                assert a.marked(n)
        if 'roots' in outputs:
            assert ints(a.get('roots')) == c.roots
        if 'old' in outputs:
            assert ints(a.get('old')) == c.old
        if 'sib' in outputs:
            assert ints(a.get('sib')) == [s for row in c.siblings for s in row]
    finally:
        a.free()
        tree.free()


@pytest.mark.parametrize('k', [3, 1])
@pytest.mark.parametrize('outputs', [s for n in range(4) for s in itertools.combinations(OUTPUTS, n)])
def test_depth0_device_arrays_equal_the_walk(ctx, p3, outputs, k):
    """the tree is its root: write j replaces what write j - 1 left (the first k writes of the case are the walk of those k alone)"""
    c = mc.case('depth0')
    assert c.depth == 0 and c.indices == [0, 0, 0]
    tree = sparse_from_dense_case(ctx, p3, c)
    a = run_dev(ctx, tree, c.indices[:k], c.values[:k], outputs)
    try:
        assert tree.root == c.roots[k - 1] and tree.level(0) == {0: c.roots[k - 1]}
        for n in OUTPUTS:
            if n not in outputs:
                assert a.marked(n)
        if 'roots' in outputs:
            assert ints(a.get('roots')) == c.roots[:k]
        if 'old' in outputs:
            assert ints(a.get('old')) == c.old[:k]
    finally:
        a.free()
        tree.free()


def _state(tree):
    return tree.root, tree.info(), [tree.level(l) for l in range(tree.depth + 1)]


def test_a_bad_index_is_refused_before_anything_is_written(ctx, p3):
    c = mc.case('hot', 65)
    tree = sparse_from_dense_case(ctx, p3, c)
    before = _state(tree)
    assert before[0] == c.root_before
    bad = list(c.indices)
    bad[40] = 1 << tree.depth
    with pytest.raises(fk.FkError) as e:
        tree.update(bad, c.values)
    assert e.value.code == 1 and 'not below 2^5' in str(e.value)
    assert _state(tree) == before
    a = DevArgs(ctx, tree.depth, bad, rows(c.values))
    try:
        with pytest.raises(fk.FkError) as e:
            tree.update_dev(a.d['idx'], a.d['new'], a.k, a.d['old'], a.d['sib'], a.d['roots'])
        assert e.value.code == 1 and 'not below 2^5' in str(e.value)
        ctx.sync()
        assert _state(tree) == before
        assert all(a.marked(n) for n in OUTPUTS)
        with pytest.raises(fk.FkError) as e:                                 # read-only proofs check their indices the same way
            tree.proofs_dev(a.d['idx'], a.k, a.d['old'], a.d['sib'])
        assert e.value.code == 1
        ctx.sync()
        assert all(a.marked(n) for n in OUTPUTS)
        with pytest.raises(fk.FkError) as e:                                 # more writes than one call takes: refused before a pointer is read
            tree.update_dev(a.d['idx'], a.d['new'], (1 << 28) + 1, None, None, None)
        assert e.value.code == 1 and '2^28' in str(e.value)
        with pytest.raises(fk.FkError) as e:
            tree.update_dev(None, a.d['new'], a.k, None, None, None)
        assert e.value.code == 1
    finally:
        a.free()
    with pytest.raises(fk.FkError) as e:
        S.SparseMerkleTree(ctx, fk.PoseidonParams(4, 8, 54), 5)
    assert e.value.code == 1 and 't = 3' in str(e.value)
    with pytest.raises(fk.FkError) as e:
        S.SparseMerkleTree(ctx, p3, 64)
    assert e.value.code == 1 and '63' in str(e.value)
    lib = S._lib()
    assert lib.fk_smt_update_dev(ctx.handle, None, None, None, 1, None, None, None) == 1
    assert lib.fk_smt_root(ctx.handle, None, None) == 1
    assert _state(tree) == before
    upd = tree.update(c.indices, c.values)                                   # the context and the tree are as they were
    assert (upd.root_before, upd.old_leaves, upd.siblings, upd.roots) == (c.root_before, c.old, c.siblings, c.roots)
    assert_stored_is_dense(tree, c)
    tree.free()


def test_an_empty_call_changes_nothing(ctx, p3):
    c = mc.case('edges')
    tree = sparse_from_dense_case(ctx, p3, c)
    before = _state(tree)
    upd = tree.update([], [])
    assert len(upd) == 0 and upd.old_leaves == [] and upd.siblings == [] and upd.roots == [] and upd.root_before == c.root_before
    tree.update_dev(None, None, 0, None, None, None)
    tree.proofs_dev(None, 0, None, None)
    assert tree.proofs([]) == ([], [])
    ctx.sync()
    assert _state(tree) == before
    tree.free()


def test_a_leaf_written_back_to_zero_stays_stored_and_the_export_checks_its_room(ctx, p3):
    tree = S.SparseMerkleTree(ctx, p3, 32)
    zero = tree.defaults
    upd = tree.update([7, 9, 7], [5, 6, 0])
    assert upd.old_leaves == [0, 0, 5] and upd.root_before == zero[32]
    assert tree.level(0) == {7: 0, 9: 6} and tree.leaves() == ([7, 9], [0, 6]) and tree.info()['leaves'] == 2
    upd = tree.update([9], [0])
    assert upd.roots == [zero[32]] and tree.root == zero[32]                 # all leaves 0 again: the empty root, with two leaves stored
    assert tree.level(0) == {7: 0, 9: 0} and tree.level(1) == {3: zero[1], 4: zero[1]} and tree.info()['leaves'] == 2
    lib, n = S._lib(), S.C.c_size_t()
    keys, vals = np.full(2, MARK, np.uint64), np.full((2, 4), MARK, np.uint64)
    assert lib.fk_smt_export_level(ctx.handle, tree.handle, 0, keys.ctypes.data, vals.ctypes.data, 1, S.C.byref(n)) == 1      # room for one of two
    assert n.value == 2 and (keys == MARK).all() and (vals == MARK).all()
    assert lib.fk_smt_export_level(ctx.handle, tree.handle, 33, None, None, 0, S.C.byref(n)) == 1                             # no such level
    assert lib.fk_smt_export_level(ctx.handle, tree.handle, 0, keys.ctypes.data, vals.ctypes.data, 2, S.C.byref(n)) == 0
    assert keys.tolist() == [7, 9] and not vals.any()
    other = fk.Context(0)                                                    # a tree is its own context's
    try:
        out = np.zeros(4, np.uint64)
        assert lib.fk_smt_root(other.handle, tree.handle, out.ctypes.data) == 1 and not out.any()
        assert lib.fk_smt_update_dev(other.handle, tree.handle, None, None, 1, None, None, None) == 1
    finally:
        other.close()
    tree.free()


def test_limbs_in_give_limbs_out(ctx, p3):
    c = mc.case('edges')
    tree = sparse_from_dense_case(ctx, p3, c)
    upd = tree.update(np.asarray(c.indices, np.uint64), rows(c.values))
    assert upd.old_leaves.shape == (7, 4) and upd.siblings.shape == (7, 3, 4) and upd.roots.shape == (7, 4) and upd.root_before.shape == (4,)
    assert ints(upd.roots) == c.roots and ints(upd.siblings) == [s for row in c.siblings for s in row] and ints(upd.old_leaves) == c.old
    assert ints(upd.roots_before()) == [c.root_before] + c.roots[:-1]
    tree.free()


# ---------------------------------------------------------------- the chained batch of tests/test_gpu_merkle_update.py
def test_six_chained_transactions_give_what_the_dense_tree_gives(ctx, p3):
    """four accounts at depth 2, six balance changes: accounts 0 and 1 (siblings), 0 again, then 2, 3 (siblings) and 2 again"""
    P3, JJ = fc.PoseidonParams(3, 8, 53), fc.JubJubBN256()
    rnd = random.Random(6)
    a_xs = [JJ.mul(JJ.g, rnd.randrange(fc.FS))[0] for _ in range(4)]
    leaves0 = [fc.poseidon([a, b], P3) for a, b in zip(a_xs, [1000, 2000, 3000, 4000])]
    txs = [(0, 900), (1, 2100), (0, 850), (2, 2500), (3, 4500), (2, 0)]
    idx, new = [t[0] for t in txs], [fc.poseidon([a_xs[t[0]], t[1]], P3) for t in txs]
    dense = ctx.merkle_tree(p3, leaves0)
    tree = S.SparseMerkleTree(ctx, p3, 2)
    try:
        populate(ctx, tree, list(enumerate(leaves0)))
        want, got = M.update(dense, p3, idx, new), tree.update(idx, new)
        assert (got.root_before, got.old_leaves, got.siblings, got.roots) == (want.root_before, want.old_leaves, want.siblings, want.roots)
        assert got.roots_before() == want.roots_before() and got.old_leaves[2] == new[0] and got.old_leaves[5] == new[3]
        walk = mc.Case(2, leaves0, idx, new)
        assert (got.old_leaves, got.siblings, got.roots) == (walk.old, walk.siblings, walk.roots)
    finally:
        dense.free(); tree.free()


# ---------------------------------------------------------------- the claim on the staging buffers
def test_updates_are_refused_during_an_early_front_and_reads_are_not():
    """the early front exists under the sorts-first schedule only, which is chosen per process: tests/_sparse_stage_child.py"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(('FK_SPMV_', 'FK_PROVE_'))}
    env['FK_PROVE_SORTS_FIRST'] = '1'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_sparse_stage_child.py')], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'SPARSE STAGE ok refused=True' in out.stdout, out.stdout[-1000:]
