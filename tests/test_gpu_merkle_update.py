"""Ordered leaf writes to a resident Poseidon Merkle tree (csrc/merkle_update.hip through fawkes_crypto_amd/merkle.py) against the
in-order walk on the oracle's poseidon (tests/merkle_cases.py): old leaves, every sibling, every root and ALL nodes of the final tree;
device-only consistency at a size the oracle cannot reach; NULL outputs, refusals, the empty call, the cached root; and one batch of
chained transactions from the update's output to a checked proof.  Every comparison is exact equality of canonical integers or bytes."""
import itertools
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc
import fixtures as fx
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import check as K
from fawkes_crypto_amd import merkle as M
from fawkes_crypto_amd import witness as W
from helpers import TOXIC
import merkle_cases as mc
from test_gpu_witness import Gadget, _BUILD, _JJ, _P3, _P4, _preimage

pytestmark = pytest.mark.gpu
R = ref.R
TOX = {k: fx.mont_fr(v) for k, v in TOXIC.items()}
MARK = 0xa5a5a5a5a5a5a5a5
OUTPUTS = ('old', 'sib', 'roots')
SUBSETS = [s for n in range(4) for s in itertools.combinations(OUTPUTS, n)]


@pytest.fixture(scope='module')
def p3():
    return fk.PoseidonParams(3, 8, 53)


def node_ints(tree):
    return fk.api._fr_ints(tree.nodes())


def assert_case(tree, upd, c):
    assert upd.root_before == c.root_before
    assert upd.old_leaves == c.old
    assert upd.siblings == c.siblings
    assert upd.roots == c.roots
    assert node_ints(tree) == c.nodes
    assert tree.n_leaves == c.n_leaves and tree.depth == c.depth


class DevArgs:
    """the writes of a case in device memory, and marked output arrays"""

    def __init__(self, ctx, depth, indices, leaves_mont):
        self.ctx, self.k, self.depth = ctx, len(indices), depth
        k = self.k
        self.sizes = dict(idx=8 * k, new=32 * k, old=32 * k, sib=32 * k * depth, roots=32 * k)
        self.d = {n: ctx.dev_alloc(max(b, 32)) for n, b in self.sizes.items()}
        if k:
            ctx.upload(self.d['idx'], np.asarray(indices, np.uint64))
            ctx.upload(self.d['new'], leaves_mont)
        for n in ('old', 'sib', 'roots'):
            if self.sizes[n]:
                ctx.upload(self.d[n], np.full(self.sizes[n] // 8, MARK, np.uint64))

    def get(self, name):
        return self.ctx.download(self.d[name], self.sizes[name], np.uint64).reshape(-1, 4) if self.sizes[name] else np.zeros((0, 4), np.uint64)

    def free(self):
        for p in self.d.values():
            self.ctx.dev_free(p)


def run_dev(ctx, p3, tree, indices, values, outputs=('old', 'sib', 'roots')):
    """fk_poseidon_merkle_update_dev with the named outputs (the others NULL) -> DevArgs (the caller frees)"""
    a = DevArgs(ctx, tree.depth, indices, fk.api._fr_rows(values, len(values)))
    try:
        M.update_dev(ctx, p3, tree.d_nodes, tree.depth, a.d['idx'], a.d['new'], a.k, *(a.d[n] if n in outputs else None for n in ('old', 'sib', 'roots')))
        ctx.sync()
    except Exception:
        a.free()
        raise
    return a


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize('name', ['depth0', 'depth1_01', 'depth1_10', 'one_index', 'alternate', 'edges'])
def test_small_cases_equal_the_walk(ctx, p3, name):
    c = mc.case(name)
    tree = ctx.merkle_tree(p3, c.leaves)
    assert tree.depth == c.depth
    upd = M.update(tree, p3, c.indices, c.values)
    assert_case(tree, upd, c)
    if name == 'edges':
        assert len(c.leaves) == 5 and tree.n_leaves == 8                  # the leaves were appended
    tree.free()


@pytest.mark.parametrize('k', [1, 63, 64, 65, 257])
def test_hot_set_host_arrays_equal_the_walk(ctx, p3, k):
    c = mc.case('hot', k)
    tree = ctx.merkle_tree(p3, c.leaves)
    assert_case(tree, M.update(tree, p3, c.indices, c.values), c)
    tree.free()


@pytest.mark.parametrize('k', [1, 63, 64, 65, 257])
def test_hot_set_device_arrays_equal_the_walk(ctx, p3, k):
    c = mc.case('hot', k)
    tree = ctx.merkle_tree(p3, c.leaves)
    a = run_dev(ctx, p3, tree, c.indices, c.values)
    try:
        assert fk.api._fr_ints(a.get('old')) == c.old
        assert fk.api._fr_ints(a.get('sib')) == [s for row in c.siblings for s in row]
        assert fk.api._fr_ints(a.get('roots')) == c.roots
        assert node_ints(tree) == c.nodes
    finally:
        a.free()
        tree.free()


def test_limbs_in_give_limbs_out(ctx, p3):
    c = mc.case('edges')
    tree = ctx.merkle_tree(p3, c.leaves)
    upd = M.update(tree, p3, np.asarray(c.indices, np.uint64), fk.api._fr_rows(c.values))
    assert upd.old_leaves.shape == (7, 4) and upd.siblings.shape == (7, 3, 4) and upd.roots.shape == (7, 4) and upd.root_before.shape == (4,)
    assert fk.api._fr_ints(upd.roots) == c.roots and fk.api._fr_ints(upd.siblings) == [s for row in c.siblings for s in row]
    assert fk.api._fr_ints(upd.roots_before()) == [c.root_before] + c.roots[:-1]
    tree.free()


# ---------------------------------------------------------------- device only: depth 12, 5000 writes
def test_depth12_5000_writes_are_consistent_on_the_device(ctx, p3):
    depth, k, n0 = 12, 5000, 3000
    rnd = random.Random(5000)
    hot = rnd.sample(range(1 << depth), 16)
    indices = [rnd.choice(hot) if j & 1 else rnd.randrange(1 << depth) for j in range(k)]
    leaves = fk.api._fr_rows(mc.values_for(n0, rnd))
    values = fk.api._fr_rows(mc.values_for(k, rnd))
    tree = ctx.merkle_tree(p3, leaves)
    assert tree.depth == depth
    root_before = tree.nodes()[-1].copy()
    a = run_dev(ctx, p3, tree, indices, values)
    d_out = ctx.dev_alloc(32 * k)
    try:
        roots = a.get('roots')
        ctx.merkle_proof_roots_dev(p3, a.d['old'], a.d['sib'], a.d['idx'], depth, k, d_out)
        got = ctx.download(d_out, 32 * k, np.uint64).reshape(-1, 4)
        assert got.tobytes() == np.concatenate([root_before.reshape(1, 4), roots[:-1]]).tobytes()
        ctx.merkle_proof_roots_dev(p3, a.d['new'], a.d['sib'], a.d['idx'], depth, k, d_out)
        assert ctx.download(d_out, 32 * k, np.uint64).tobytes() == roots.tobytes()
        final = np.zeros((1 << depth, 4), np.uint64)
        final[:n0] = leaves
        for i, v in zip(indices, values):
            final[i] = v
        rebuilt = ctx.merkle_tree(p3, final)
        assert tree.nodes().tobytes() == rebuilt.nodes().tobytes()
        rebuilt.free()
    finally:
        ctx.dev_free(d_out)
        a.free()
        tree.free()


# ---------------------------------------------------------------- NULL outputs, refusals, the empty call, the cached root
@pytest.mark.parametrize('outputs', SUBSETS)
def test_null_outputs_leave_the_same_tree(ctx, p3, outputs):
    c = mc.case('hot', 65)
    tree = ctx.merkle_tree(p3, c.leaves)
    a = run_dev(ctx, p3, tree, c.indices, c.values, outputs)
    try:
        assert node_ints(tree) == c.nodes
        for n in OUTPUTS:                                               # what was not asked for was not written
            if n not in outputs:
                assert (a.get(n) == MARK).all()
        if 'roots' in outputs:
            assert fk.api._fr_ints(a.get('roots')) == c.roots
        if 'old' in outputs:
            assert fk.api._fr_ints(a.get('old')) == c.old
        if 'sib' in outputs:
            assert fk.api._fr_ints(a.get('sib')) == [s for row in c.siblings for s in row]
    finally:
        a.free()
        tree.free()


@pytest.mark.parametrize('k', [3, 1])
@pytest.mark.parametrize('outputs', SUBSETS)
def test_depth0_device_arrays_equal_the_walk(ctx, p3, outputs, k):
    """the tree is its root: write j replaces what write j - 1 left (the first k writes of the case are the walk of those k alone)"""
    c = mc.case('depth0')
    assert c.depth == 0 and c.indices == [0, 0, 0]
    tree = ctx.merkle_tree(p3, c.leaves)
    a = run_dev(ctx, p3, tree, c.indices[:k], c.values[:k], outputs)
    try:
        assert node_ints(tree) == [c.roots[k - 1]]
        for n in OUTPUTS:
            if n not in outputs:
                assert (a.get(n) == MARK).all()
        if 'roots' in outputs:
            assert fk.api._fr_ints(a.get('roots')) == c.roots[:k]
        if 'old' in outputs:
            assert fk.api._fr_ints(a.get('old')) == c.old[:k]
    finally:
        a.free()
        tree.free()


def test_a_bad_index_is_refused_before_anything_is_written(ctx, p3):
    c = mc.case('hot', 65)
    tree = ctx.merkle_tree(p3, c.leaves)
    root = tree.root
    before = tree.nodes().tobytes()
    bad = list(c.indices)
    bad[40] = 1 << tree.depth
    with pytest.raises(fk.FkError) as e:
        M.update(tree, p3, bad, c.values)
    assert e.value.code == 1 and 'not below 2^5' in str(e.value)
    assert tree.nodes().tobytes() == before and tree.n_leaves == 20 and tree._root == root
    a = DevArgs(ctx, tree.depth, bad, fk.api._fr_rows(c.values))
    try:
        with pytest.raises(fk.FkError):
            M.update_dev(ctx, p3, tree.d_nodes, tree.depth, a.d['idx'], a.d['new'], a.k, a.d['old'], a.d['sib'], a.d['roots'])
        ctx.sync()
        assert tree.nodes().tobytes() == before
        assert all((a.get(n) == MARK).all() for n in ('old', 'sib', 'roots'))
    finally:
        a.free()
    p4 = fk.PoseidonParams(4, 8, 54)
    with pytest.raises(fk.FkError) as e:
        M.update(tree, p4, c.indices, c.values)
    assert e.value.code == 1 and 't = 3' in str(e.value)
    with pytest.raises(fk.FkError):                                      # no tree this deep is in device memory
        M.update_dev(ctx, p3, tree.d_nodes, 41, tree.d_nodes, tree.d_nodes, 1, None, None, None)
    assert tree.nodes().tobytes() == before
    assert_case(tree, M.update(tree, p3, c.indices, c.values), c)        # the context and the tree are as they were
    tree.free()


def test_an_empty_call_changes_nothing(ctx, p3):
    c = mc.case('edges')
    tree = ctx.merkle_tree(p3, c.leaves)
    root = tree.root
    before = tree.nodes().tobytes()
    upd = M.update(tree, p3, [], [])
    assert len(upd) == 0 and upd.old_leaves == [] and upd.siblings == [] and upd.roots == [] and upd.root_before == c.root_before
    M.update_dev(ctx, p3, tree.d_nodes, tree.depth, None, None, 0, None, None, None)
    ctx.sync()
    assert tree.nodes().tobytes() == before and tree.n_leaves == 5 and tree._root == root
    tree.free()


def test_the_cached_root_is_dropped(ctx, p3):
    c = mc.case('one_index')
    tree = ctx.merkle_tree(p3, c.leaves)
    assert tree.root == c.root_before and tree._root is not None
    upd = M.update(tree, p3, c.indices, c.values)
    assert tree.root == upd.roots[-1] == c.roots[-1]
    tree.free()


# ---------------------------------------------------------------- end to end: a batch whose roots chain
def _tx_row(sk, bal_old, bal_new, index, siblings, root_old, root_new, rho):
    """the given row of rollup_tx_circuit(..., 2) (tests/test_gpu_witness.py: _rollup_given) with the path and the roots the TREE gives"""
    a_x = _JJ.mul(_JJ.g, sk)[0]
    leaf_new = fc.poseidon([a_x, bal_new], _P3)
    s, r_x, _ = fc.eddsaposeidon_sign(sk, leaf_new, rho, _P4, _JJ)
    return [root_old, root_new, a_x, bal_old, bal_new, *siblings, index & 1, index >> 1, s, r_x, *_preimage(a_x), *_preimage(r_x)]


def test_six_chained_transactions_from_the_update_to_the_checked_proof(ctx, p3):
    """Four accounts, six balance changes: accounts 0 and 1 (siblings), account 0 again, then 2, 3 (siblings) and 2 again.  The rows of
    the six copies take their siblings and roots from merkle.update; the checked prover finds no bad copy and the public inputs chain.
    Then the tree is given the list with writes 0 and 2 swapped (both to account 0) while every row keeps the transaction it had at its
    position: the copies the check names are those whose transaction is no longer the write the tree applied there -- 0 and 2, as the
    in-order walk says; copy 1 (the sibling account, whose path now holds the other value of account 0) and the later copies hold."""
    rnd = random.Random(6)
    sks = [rnd.randrange(fc.FS) for _ in range(4)]
    a_xs = [_JJ.mul(_JJ.g, sk)[0] for sk in sks]
    balance = [1000, 2000, 3000, 4000]
    leaves0 = [fc.poseidon([a, b], _P3) for a, b in zip(a_xs, balance)]
    txs, bal = [], list(balance)                                   # (account, old balance, new balance)
    for acct, new in [(0, 900), (1, 2100), (0, 850), (2, 2500), (3, 4500), (2, 0)]:
        txs.append((acct, bal[acct], new))
        bal[acct] = new
    rhos = [rnd.randrange(fc.FS) for _ in txs]
    new_leaf = lambda t: fc.poseidon([a_xs[t[0]], t[2]], _P3)

    def rows_for(order):
        """the tree applies txs[order[j]] at position j; row j is transaction j's own"""
        tree = ctx.merkle_tree(p3, leaves0)
        upd = M.update(tree, p3, [txs[i][0] for i in order], [new_leaf(txs[i]) for i in order])
        tree.free()
        before = upd.roots_before()
        rows = [_tx_row(sks[t[0]], t[1], t[2], txs[order[j]][0], upd.siblings[j], before[j], upd.roots[j], rhos[j]) for j, t in enumerate(txs)]
        return upd, rows

    g = Gadget(*_BUILD['rollup2'])
    copies = len(txs)
    dp = W.load(ctx, g.prog)
    dk, _ = ctx.setup(g.r1cs, copies=copies, **TOX)
    dr = ctx.load_r1cs(g.r1cs, copies=copies)
    r, s = fx.mont_fr(0x6a), fx.mont_fr(0x6b)
    try:
        assert g.prog.n_given == 15
        upd, rows = rows_for(range(copies))
        want = mc.Case(2, leaves0, [t[0] for t in txs], [new_leaf(t) for t in txs])
        assert (upd.old_leaves, upd.siblings, upd.roots) == (want.old, want.siblings, want.roots)
        assert upd.old_leaves == [fc.poseidon([a_xs[t[0]], t[1]], _P3) for t in txs]
        _, rep = K.prove_given_checked(ctx, dk, dr, dp, rows, r, s)
        assert rep.ok and rep.n_groups == copies and rep.bad_groups().tolist() == []
        assert rows[0][0] == want.root_before and all(rows[j][1] == rows[j + 1][0] for j in range(copies - 1))      # new_root[j] == old_root[j + 1]
        # writes 0 and 2 swapped in the list, the transactions of the rows where they were
        order = [2, 1, 0, 3, 4, 5]
        upd2, rows2 = rows_for(order)
        walk2 = mc.Case(2, leaves0, [txs[i][0] for i in order], [new_leaf(txs[i]) for i in order])
        affected = [j for j, t in enumerate(txs) if (fc.poseidon([a_xs[t[0]], t[1]], _P3), new_leaf(t)) != (walk2.old[j], walk2.values[j])]
        assert affected == [0, 2] and upd2.roots == walk2.roots and upd2.roots[-1] != upd.roots[-1]
        _, rep2 = K.prove_given_checked(ctx, dk, dr, dp, rows2, r, s)
        assert not rep2.ok and rep2.bad_groups().tolist() == affected
    finally:
        dr.free(); dk.free(); dp.free()
