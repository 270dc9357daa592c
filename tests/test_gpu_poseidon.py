"""Device Poseidon (csrc/poseidon.hip) against the Python restatement of native/poseidon.rs in oracle/fawkes_circuit.py: batch hashes, the
sponge, Merkle trees node by node, sibling gathers and proof roots.  Every comparison is exact integer equality of canonical values."""
import functools
import json
import os
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc

pytestmark = pytest.mark.gpu

R = ref.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'poseidon_merkle_golden.json')
DIMS = {2: (2, 8, 56), 3: (3, 8, 53), 4: (4, 8, 54), 5: (5, 8, 57), 8: (8, 8, 60)}
TAIL_NODES = 1024        # the level width under which a single-workgroup tail kernel was tried (and dropped: DESIGN 3.6); 2 * 1024 + 1 leaves stay a case


@functools.lru_cache(maxsize=None)
def oracle_params(t):
    return fc.PoseidonParams(*DIMS[t])


@functools.lru_cache(maxsize=None)
def device_params(t):
    import fawkes_crypto_amd as fk
    return fk.PoseidonParams(*DIMS[t])


def edge_rows(k, n, seed):
    """n rows of k inputs: all-zero, all-(r - 1), all-one and mixed edge rows first, seeded random values behind them"""
    rnd = random.Random(seed)
    rows = [[0] * k, [R - 1] * k, [1] * k, [(0, 1, R - 1)[(j + 1) % 3] for j in range(k)]]
    while len(rows) < n:
        rows.append([rnd.choice((0, 1, R - 1)) if rnd.random() < 0.1 else rnd.randrange(R) for _ in range(k)])
    return rows[:n]


def mont_limbs(values):
    from fawkes_crypto_amd import api
    return api._fr_rows(values)


def canon(limbs):
    from fawkes_crypto_amd import api
    return api._fr_ints(limbs)


def hash_dev(ctx, params, rows, k):
    """the same batch through fk_poseidon_hash_batch_dev: resident inputs, resident outputs"""
    n = len(rows)
    d_in, d_out = ctx.dev_alloc(32 * n * k), ctx.dev_alloc(32 * n)
    try:
        ctx.upload(d_in, mont_limbs(rows))
        ctx.poseidon_dev(params, d_in, k, n, d_out)
        ctx.sync()
        return canon(ctx.download(d_out, 32 * n, np.uint64))
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


@pytest.mark.parametrize('t', [2, 3, 4, 5, 8])
def test_hash_batch_matches_oracle(ctx, t):
    """every n_inputs in 1 .. t - 1; n = 1, 63, 64, 65 (a partial wave on either side of a full one) and 257 (a partial second workgroup).
    The reference is computed once for 257 rows; the shorter batches are its prefixes."""
    op, dp = oracle_params(t), device_params(t)
    for k in range(1, t):
        rows = edge_rows(k, 257, 1000 * t + k)
        want = [fc.poseidon(r, op) for r in rows]
        for n in (1, 63, 64, 65, 257):
            assert ctx.poseidon(dp, rows[:n]) == want[:n], (t, k, n, 'host arrays')
            assert hash_dev(ctx, dp, rows[:n], k) == want[:n], (t, k, n, 'device arrays')
    assert ctx.poseidon(dp, []) == []          # n == 0 is a no-op
    limbs = ctx.poseidon(dp, mont_limbs(rows[:5]).reshape(5, t - 1, 4))       # limb arrays in, limbs out
    assert limbs.dtype == np.uint64 and canon(limbs) == want[:5]


def sponge_ref(msg, p):
    """poseidon.rs:102-110 on top of the oracle's permutation"""
    state = [0] * p.t
    stream = [len(msg)] + list(msg)
    for off in range(0, len(stream), p.t - 1):
        for j, v in enumerate(stream[off:off + p.t - 1]):
            state[j] = (state[j] + v) % R
        state = fc.poseidon_perm(state, p)
    return state[0]


@pytest.mark.parametrize('t', [3, 5])
def test_sponge_matches_oracle(ctx, t):
    op, dp = oracle_params(t), device_params(t)
    for ln in (0, 1, t - 2, t - 1, t, 2 * (t - 1) + 1):
        msgs = edge_rows(ln, 65, 77 * t + ln) if ln else [[] for _ in range(65)]
        assert ctx.poseidon_sponge(dp, msgs) == [sponge_ref(m, op) for m in msgs], (t, ln)


@functools.lru_cache(maxsize=None)
def zero_roots():
    """root of the all-zero subtree of every height"""
    z = [0]
    for _ in range(16):
        z.append(fc.poseidon([z[-1], z[-1]], oracle_params(3)))
    return z


@functools.lru_cache(maxsize=None)
def tree_ref(n_leaves):
    """(leaves, levels): the Python tree, all-zero subtrees memoised; computed once per size, shared by the tests, never modified"""
    rnd = random.Random(31337 + n_leaves)
    leaves = [rnd.randrange(R) for _ in range(n_leaves)]
    for pos, v in ((1, 0), (2, R - 1), (3, 1), (n_leaves - 2, 0)):          # edge values among seeded random ones
        if 0 < pos < n_leaves:
            leaves[pos] = v
    leaves = tuple(leaves)
    depth = max(n_leaves - 1, 0).bit_length()
    z = zero_roots()
    level = list(leaves) + [0] * ((1 << depth) - n_leaves)
    levels = [tuple(level)]
    for h in range(depth):
        level = [z[h + 1] if (level[2 * i], level[2 * i + 1]) == (z[h], z[h]) else fc.poseidon([level[2 * i], level[2 * i + 1]], oracle_params(3))
                 for i in range(len(level) // 2)]
        levels.append(tuple(level))
    return leaves, tuple(levels)


@pytest.mark.parametrize('n_leaves', [1, 2, 3, 5, 64, 65, 1000, 2 * TAIL_NODES + 1])
def test_tree_node_by_node(ctx, n_leaves):
    """one leaf (the root is the leaf) up to 2 * TAIL_NODES + 1 leaves, which pad to 4096: levels of 8, 4, 2 and 1 workgroups, then partial ones"""
    leaves, levels = tree_ref(n_leaves)
    dp = device_params(3)
    assert ctx.merkle_root(dp, list(leaves)) == levels[-1][0]
    tree = ctx.merkle_tree(dp, list(leaves))
    try:
        assert tree.depth == len(levels) - 1 and tree.n_nodes == sum(len(lv) for lv in levels)
        assert canon(tree.nodes()) == [v for lv in levels for v in lv]
        assert tree.root == levels[-1][0]
    finally:
        tree.free()


def test_proofs_from_a_tree(ctx):
    leaves, levels = tree_ref(1000)
    dp = device_params(3)
    idx = [0, 1, 511, 512, 999, 1000, 1023]
    tree = ctx.merkle_tree(dp, list(leaves))
    try:
        sib, got_idx = tree.proofs(idx)
        assert got_idx == idx
        assert sib == [[levels[j][(i >> j) ^ 1] for j in range(tree.depth)] for i in idx]
        padded = levels[0]
        roots = ctx.merkle_proof_roots(dp, [padded[i] for i in idx], sib, idx, tree.depth)
        assert roots == [levels[-1][0]] * len(idx) == [tree.root] * len(idx)
    finally:
        tree.free()


def test_proof_roots_match_oracle_and_golden(ctx):
    op, dp = oracle_params(3), device_params(3)
    g = json.load(open(GOLDEN))
    rnd = random.Random(g['seed'])                       # the committed instance: leaf, 32 siblings, 32 path bits (its _doc)
    leaves = [rnd.randrange(R)]
    sibs = [[rnd.randrange(R) for _ in range(32)]]
    paths = [[rnd.randrange(2) for _ in range(32)]]
    rnd = random.Random(64032)
    for k in range(64):
        leaves.append(rnd.choice((0, 1, R - 1)) if k < 3 else rnd.randrange(R))
        sibs.append([rnd.randrange(R) for _ in range(32)])
        paths.append([rnd.randrange(2) for _ in range(32)])
    idx = [sum(b << j for j, b in enumerate(p)) for p in paths]
    got = ctx.merkle_proof_roots(dp, leaves, sibs, idx, 32)
    assert '%064x' % got[0] == g['root']
    assert got[1:] == [fc.poseidon_merkle_proof_root(l, s, p, op) for l, s, p in zip(leaves[1:], sibs[1:], paths[1:])]
    # resident form, same bytes
    n = len(leaves)
    d_l, d_s, d_i, d_o = ctx.dev_alloc(32 * n), ctx.dev_alloc(32 * 32 * n), ctx.dev_alloc(8 * n), ctx.dev_alloc(32 * n)
    try:
        ctx.upload(d_l, mont_limbs(leaves)); ctx.upload(d_s, mont_limbs(sibs)); ctx.upload(d_i, np.array(idx, np.uint64))
        ctx.merkle_proof_roots_dev(dp, d_l, d_s, d_i, 32, n, d_o)
        ctx.sync()
        assert canon(ctx.download(d_o, 32 * n, np.uint64)) == got
    finally:
        for d in (d_l, d_s, d_i, d_o):
            ctx.dev_free(d)
    assert ctx.merkle_proof_roots(dp, leaves[:5], [], [0] * 5, 0) == leaves[:5]          # depth 0: the leaf


def test_errors_are_reported_and_the_context_goes_on(ctx):
    import fawkes_crypto_amd as fk
    p3, p4 = device_params(3), device_params(4)
    probe = [[3, 4]]
    want = [fc.poseidon(probe[0], oracle_params(3))]

    def bad_arg(call):
        with pytest.raises(fk.FkError) as e:
            call()
        assert e.value.code == 1, e.value                        # FK_ERR_BAD_ARG
        assert ctx.poseidon(p3, probe) == want                   # ... and the context still hashes correctly

    bad_arg(lambda: ctx.poseidon(p3, [[1, 2, 3]]))               # n_inputs = t
    bad_arg(lambda: ctx.poseidon(p4, [[1, 2, 3, 4]]))
    bad_arg(lambda: ctx.merkle_root(p3, []))                     # n_leaves = 0
    bad_arg(lambda: ctx.merkle_tree(p3, []))
    bad_arg(lambda: ctx.merkle_root(p4, [1, 2, 3]))              # tree calls with t = 4 parameters
    bad_arg(lambda: ctx.merkle_tree(p4, [1, 2, 3]))
    bad_arg(lambda: ctx.merkle_proof_roots(p4, [1], [[2]], [0], 1))
    bad_arg(lambda: ctx.merkle_proof_roots(p3, [1], [[2] * 65], [0], 65))        # depth > 64
    leaves, levels = tree_ref(5)
    tree = ctx.merkle_tree(p3, list(leaves))
    try:
        for idx in ([8], [0, 1 << 40, 1], [(1 << 64) - 1]):      # a proof index >= 2^depth: found on the device, never read
            bad_arg(lambda: tree.proofs(idx))
        sib, _ = tree.proofs([7])
        assert sib == [[levels[j][(7 >> j) ^ 1] for j in range(3)]]
    finally:
        tree.free()
    with pytest.raises(fk.FkError) as e:                         # t = 7 is within 2..8 but has no kernel: reported, not a fall-back
        ctx.poseidon(fk.PoseidonParams(7, 2, 1), [[1]])
    assert e.value.code == 8
    assert ctx.poseidon(p3, probe) == want
