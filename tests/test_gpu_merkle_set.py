"""Bulk leaf writes to the sparse and the dense Merkle tree on the device (csrc/merkle_plan.hpp through fawkes_crypto_amd/merkle_set.py):
the final state of the ordered update and the new root.  Every case of tests/merkle_cases.py against the dense walk and the deep cases
of tests/sparse_merkle_cases.py against the sparse walk, stored nodes included; three leaves by hand; at a size the oracle cannot reach
the ordered update of the same list, byte for byte on every level, and the number of nodes hashed per level against numpy's count of
the distinct ones; updates and sets mixed on one tree; the restore of a saved tree; refusals and the empty call.  Every comparison is
exact equality of canonical integers or bytes."""
import random

import numpy as np
import pytest

import fawkes_crypto_amd as fk
from fawkes_crypto_amd import merkle as M
from fawkes_crypto_amd import merkle_set as MS
from fawkes_crypto_amd import sparse_merkle as S
import merkle_cases as mc
import sparse_merkle_cases as sc

pytestmark = pytest.mark.gpu
MARK = 0xa5a5a5a5a5a5a5a5
ints = fk.api._fr_ints
rows = fk.api._fr_rows
CASES = [('depth0', 0), ('depth1_01', 0), ('depth1_10', 0), ('one_index', 0), ('alternate', 0), ('edges', 0)] + [('hot', k) for k in (1, 63, 64, 65, 257)]


@pytest.fixture(scope='module')
def p3():
    return fk.PoseidonParams(3, 8, 53)


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


def state(tree):
    return tree.root, tree.info(), [tree.level(l) for l in range(tree.depth + 1)]


class Dev:
    """named device arrays, freed together"""

    def __init__(self, ctx, **sizes):
        self.ctx, self.sizes = ctx, sizes
        self.d = {n: ctx.dev_alloc(max(b, 32)) for n, b in sizes.items()}

    def __getitem__(self, name):
        return self.d[name]

    def mark(self, name):
        self.ctx.upload(self.d[name], np.full(self.sizes[name] // 8, MARK, np.uint64))

    def get(self, name):
        return self.ctx.download(self.d[name], self.sizes[name], np.uint64)

    def free(self):
        for p in self.d.values():
            self.ctx.dev_free(p)


def mixture(rnd, bits, run, uniform, repeats):
    """a contiguous run, uniform indices below 2^bits, and repeats of indices already in the list; shuffled"""
    start = rnd.randrange((1 << bits) - run)
    idx = list(range(start, start + run)) + [rnd.randrange(1 << bits) for _ in range(uniform)]
    idx += [rnd.choice(idx) for _ in range(repeats)]
    rnd.shuffle(idx)
    return np.asarray(idx, np.uint64)


# ================================================================ sparse
@pytest.mark.parametrize('name,k', CASES)
def test_sparse_every_dense_case_equals_the_walk(ctx, p3, name, k):
    c = mc.case(name, k)
    tree = S.SparseMerkleTree(ctx, p3, c.depth)
    assert tree.set(list(range(len(c.leaves))), c.leaves) == c.root_before
    assert tree.set(c.indices, c.values) == c.nodes[-1] == c.roots[-1]
    assert_stored_is_dense(tree, c)
    assert_levels(tree, sc.from_dense(c).levels)            # the same SET of nodes as the ordered update stores, leaves written as 0 included
    tree.free()


@pytest.mark.parametrize('name', ['deep32', 'deep63'])
def test_sparse_deep_cases_equal_the_sparse_walk(ctx, p3, name):
    c = sc.case(name)
    tree = S.SparseMerkleTree(ctx, p3, c.depth)
    assert tree.set([i for i, _ in c.initial], [v for _, v in c.initial]) == c.root_before
    assert tree.set(c.indices, c.values) == c.roots[-1]
    assert_levels(tree, c.levels)
    assert tree.root == c.roots[-1]
    info = tree.info()
    assert info['leaves'] == len(c.levels[0]) and info['nodes'] == sum(len(lv) for lv in c.levels[:c.depth])
    tree.free()


def test_sparse_three_leaves_by_hand(ctx, p3):
    """depth 2.  set([0]): every sibling a default.  set([1]): the sibling (leaf 0) is stored and not in the list.  set([2, 3]): both
    children of a parent are in the list, and the parent's sibling is stored"""
    rnd = random.Random(3)
    tree, walk = S.SparseMerkleTree(ctx, p3, 2), sc.SparseWalk(2)
    for idx in ([0], [1], [2, 3]):
        vals = [rnd.randrange(1, mc.R) for _ in idx]
        walk.walk(idx, vals)
        assert tree.set(idx, vals) == walk.root
        assert tree.root == walk.root
        assert_levels(tree, walk.levels)
    assert tree.info()['leaves'] == 4 and tree.info()['nodes'] == 6
    tree.free()


def test_sparse_70000_writes_equal_the_ordered_update_and_hash_each_node_once(ctx, p3):
    depth, k = 32, 70000
    idx = mixture(random.Random(70000), depth, 40000, 20000, 10000)
    assert len(idx) == k and len(np.unique(idx)) < k - 5000
    a, b = S.SparseMerkleTree(ctx, p3, depth, 0), S.SparseMerkleTree(ctx, p3, depth, 0)         # the smallest tables: every level grows
    d = Dev(ctx, idx=8 * k, new=32 * k, root=32)
    try:
        ctx.upload(d['idx'], idx)
        ctx.gen_scalars_dev(d['new'], k, 7)
        d.mark('root')
        _, _, distinct = MS.set_sparse_timed_dev(a, d['idx'], d['new'], k, d['root'])
        b.update_dev(d['idx'], d['new'], k, None, None, None)
        root = b.root_limbs()
        assert a.root_limbs().tobytes() == root.tobytes() == d.get('root').tobytes()
        for l in range(depth + 1):
            ka, va = a.level_limbs(l)
            kb, vb = b.level_limbs(l)
            assert ka.tobytes() == kb.tobytes() and va.tobytes() == vb.tobytes(), l
        # one hash per node: what each level stored and hashed is the number of its distinct touched nodes, counted here by numpy
        assert distinct == [len(np.unique(idx >> np.uint64(l))) for l in range(depth + 1)]
        assert distinct[depth] == 1 and distinct[0] < k and sum(distinct[1:]) < k * depth // 2
        assert a.info() == b.info() and a.info()['leaves'] == distinct[0] and a.info()['nodes'] == sum(distinct[:depth])
    finally:
        d.free()
        a.free(); b.free()


def test_sparse_updates_and_sets_mix_on_one_tree(ctx, p3):
    """update, set, update, proofs against a twin driven by updates alone: the set grows every table of a tree that started at the
    smallest ones, and the update behind it must see the counts and bounds the set left"""
    depth = 32
    rnd = random.Random(32)
    pool = [rnd.randrange(1 << depth) for _ in range(150)] + list(range(1000, 1040))
    batches = [([rnd.choice(pool) for _ in range(n)], [rnd.randrange(mc.R) for _ in range(n)]) for n in (40, 120, 60)]
    tree, twin = S.SparseMerkleTree(ctx, p3, depth, 0), S.SparseMerkleTree(ctx, p3, depth, 0)
    try:
        tree.update(*batches[0])
        twin.update(*batches[0])
        assert tree.set(*batches[1]) == twin.update(*batches[1]).roots[-1]
        assert tree.info() == twin.info()
        got, want = tree.update(*batches[2]), twin.update(*batches[2])
        assert (got.root_before, got.old_leaves, got.siblings, got.roots) == (want.root_before, want.old_leaves, want.siblings, want.roots)
        ask = pool[::7] + [5, (1 << depth) - 1]
        assert tree.proofs(ask) == twin.proofs(ask)
        assert state(tree) == state(twin)
    finally:
        tree.free(); twin.free()


def test_sparse_restore_reproduces_a_saved_tree(ctx, p3):
    depth = 32
    old = S.SparseMerkleTree(ctx, p3, depth)
    old.update([7, 9, 7, 1 << 31, 8], [5, 6, 0, 11, 12])                      # leaf 7 is written back to 0 and stays stored
    assert old.leaves() == ([7, 8, 9, 1 << 31], [0, 12, 6, 11])
    new = MS.restore(ctx, p3, depth, *old.leaves())
    also = S.SparseMerkleTree.restore(ctx, p3, depth, *old.leaves(), expected_leaves=100)
    try:
        for t in (new, also):
            assert isinstance(t, S.SparseMerkleTree) and t.root == old.root
            assert all(t.level(l) == old.level(l) for l in range(depth + 1))
            assert t.info()['leaves'] == old.info()['leaves'] == 4 and t.info()['nodes'] == old.info()['nodes']
    finally:
        old.free(); new.free(); also.free()


def test_sparse_refusals_and_edges(ctx, p3):
    c = mc.case('hot', 65)
    tree = S.SparseMerkleTree(ctx, p3, c.depth)
    tree.set(list(range(len(c.leaves))), c.leaves)
    before = state(tree)
    assert before[0] == c.root_before
    lib, k = MS._lib(), len(c.indices)
    bad = list(c.indices)
    bad[40] = 1 << tree.depth
    d = Dev(ctx, idx=8 * k, bad=8 * k, new=32 * k, root=32)
    try:
        ctx.upload(d['idx'], np.asarray(c.indices, np.uint64))
        ctx.upload(d['bad'], np.asarray(bad, np.uint64))
        ctx.upload(d['new'], rows(c.values))
        d.mark('root')
        # k = 0 touches nothing, whatever the pointers
        tree.set_dev(None, None, 0, d['root'])
        assert MS.set_sparse_timed_dev(tree, None, None, 0, d['root']) == (0.0, 0.0, [])
        assert tree.set([], []) == c.root_before
        ctx.sync()
        assert (d.get('root') == MARK).all() and state(tree) == before
        # an index equal to 2^depth: refused, nothing written
        with pytest.raises(fk.FkError) as e:
            tree.set(bad, c.values)
        assert e.value.code == 1 and 'not below 2^5' in str(e.value)
        with pytest.raises(fk.FkError) as e:
            tree.set_dev(d['bad'], d['new'], k, d['root'])
        assert e.value.code == 1 and 'not below 2^5' in str(e.value)
        distinct = np.full(tree.depth + 1, MARK, np.uint64)
        assert lib.fk_smt_set_timed_dev(ctx.handle, tree.handle, d['bad'], d['new'], k, d['root'], None, distinct.ctypes.data) == 1
        ctx.sync()
        assert (d.get('root') == MARK).all() and (distinct == MARK).all() and state(tree) == before
        # more writes than one call takes: refused before a pointer is read; a null array; a null tree; a tree of another context
        with pytest.raises(fk.FkError) as e:
            tree.set_dev(d['idx'], d['new'], (1 << 28) + 1, d['root'])
        assert e.value.code == 1 and '2^28' in str(e.value)
        assert lib.fk_smt_set_dev(ctx.handle, tree.handle, None, d['new'], k, d['root']) == 1
        assert lib.fk_smt_set_dev(ctx.handle, tree.handle, d['idx'], None, k, d['root']) == 1
        assert lib.fk_smt_set_dev(ctx.handle, None, d['idx'], d['new'], k, d['root']) == 1
        other = fk.Context(0)
        try:
            assert lib.fk_smt_set_dev(other.handle, tree.handle, d['idx'], d['new'], k, d['root']) == 1
            h_idx, h_new, out = np.asarray(c.indices, np.uint64), rows(c.values), np.full(4, MARK, np.uint64)
            assert lib.fk_smt_set(other.handle, tree.handle, h_idx.ctypes.data, h_new.ctypes.data, k, out.ctypes.data) == 1
            assert (out == MARK).all()
        finally:
            other.close()
        ctx.sync()
        assert (d.get('root') == MARK).all() and state(tree) == before
        # a NULL root is accepted, and the tree is the one the walk says
        tree.set_dev(d['idx'], d['new'], k, None)
        ctx.sync()
        assert (d.get('root') == MARK).all()
        assert_stored_is_dense(tree, c)
        tree.set_dev(d['idx'], d['new'], k, d['root'])                      # the same writes again: every node overwritten with what it holds
        assert ints(d.get('root').reshape(1, 4)) == [c.nodes[-1]]
        assert_stored_is_dense(tree, c)
    finally:
        d.free()
        tree.free()


# ================================================================ dense
@pytest.mark.parametrize('name,k', CASES)
def test_dense_every_case_leaves_the_walks_nodes(ctx, p3, name, k):
    c = mc.case(name, k)
    tree = ctx.merkle_tree(p3, c.leaves)
    assert tree.depth == c.depth and tree.root == c.root_before
    assert MS.set_dense(tree, p3, c.indices, c.values) == c.nodes[-1]
    assert tree.nodes().tobytes() == rows(c.nodes).tobytes()
    assert tree.n_leaves == c.n_leaves and tree.root == c.roots[-1]
    tree.free()


def test_dense_70000_writes_equal_the_ordered_update_and_a_rebuild(ctx, p3):
    depth, k = 17, 70000
    n = 1 << depth
    idx = mixture(random.Random(17), depth, 40000, 20000, 10000)
    d = Dev(ctx, idx=8 * k, new=32 * k, leaves=32 * n, a=32 * (2 * n - 1), b=32 * (2 * n - 1), c=32 * (2 * n - 1))
    try:
        ctx.upload(d['idx'], idx)
        ctx.gen_scalars_dev(d['new'], k, 7)
        ctx.gen_scalars_dev(d['leaves'], n, 8)
        ctx.merkle_tree_dev(p3, d['leaves'], n, d['a'])
        ctx.dev_copy(d['b'], d['a'], 32 * (2 * n - 1))
        _, _, distinct = MS.set_dense_timed_dev(ctx, p3, d['a'], depth, d['idx'], d['new'], k)
        M.update_dev(ctx, p3, d['b'], depth, d['idx'], d['new'], k, None, None, None)
        ctx.sync()
        final = d.get('leaves').reshape(n, 4)
        new = d.get('new').reshape(k, 4)
        for j in range(k):                                                  # in list order: the last write to an index wins
            final[int(idx[j])] = new[j]
        ctx.upload(d['leaves'], final)
        ctx.merkle_tree_dev(p3, d['leaves'], n, d['c'])
        ctx.sync()
        nodes = d.get('a').tobytes()
        assert nodes == d.get('b').tobytes()
        assert nodes == d.get('c').tobytes()
        assert distinct == [len(np.unique(idx >> np.uint64(l))) for l in range(depth + 1)]
    finally:
        d.free()


def test_dense_refusals_leave_the_nodes_as_they_were(ctx, p3):
    c = mc.case('hot', 65)
    tree = ctx.merkle_tree(p3, c.leaves)
    root, before = tree.root, tree.nodes().tobytes()
    bad = list(c.indices)
    bad[40] = 1 << tree.depth
    with pytest.raises(fk.FkError) as e:
        MS.set_dense(tree, p3, bad, c.values)
    assert e.value.code == 1 and 'not below 2^5' in str(e.value)
    assert tree.nodes().tobytes() == before and tree.n_leaves == 20 and tree._root == root
    with pytest.raises(fk.FkError) as e:
        MS.set_dense(tree, fk.PoseidonParams(4, 8, 54), c.indices, c.values)
    assert e.value.code == 1 and 't = 3' in str(e.value)
    k = len(c.indices)
    d = Dev(ctx, idx=8 * k, new=32 * k)
    try:
        ctx.upload(d['idx'], np.asarray(bad, np.uint64))
        ctx.upload(d['new'], rows(c.values))
        with pytest.raises(fk.FkError):
            MS.set_dense_dev(ctx, p3, tree.d_nodes, tree.depth, d['idx'], d['new'], k)
        with pytest.raises(fk.FkError):                                      # no tree this deep is in device memory
            MS.set_dense_dev(ctx, p3, tree.d_nodes, 41, d['idx'], d['new'], 1)
        with pytest.raises(fk.FkError) as e:
            MS.set_dense_dev(ctx, p3, tree.d_nodes, tree.depth, d['idx'], d['new'], (1 << 28) + 1)
        assert '2^28' in str(e.value)
        lib = MS._lib()
        assert lib.fk_poseidon_merkle_set_dev(ctx.handle, p3.handle, None, tree.depth, d['idx'], d['new'], k) == 1
        assert lib.fk_poseidon_merkle_set_dev(ctx.handle, p3.handle, tree.d_nodes, tree.depth, None, d['new'], k) == 1
        assert lib.fk_poseidon_merkle_set_dev(ctx.handle, None, tree.d_nodes, tree.depth, d['idx'], d['new'], k) == 1
        MS.set_dense_dev(ctx, p3, tree.d_nodes, tree.depth, None, None, 0)   # the empty call
        assert MS.set_dense(tree, p3, [], []) == c.root_before
        ctx.sync()
        assert tree.nodes().tobytes() == before and tree.n_leaves == 20 and tree._root == root
    finally:
        d.free()
    assert MS.set_dense(tree, p3, c.indices, c.values) == c.nodes[-1]        # the context and the tree are as they were
    assert ints(tree.nodes()) == c.nodes
    tree.free()
