"""Shared by tests/test_merkle_update_host.py and tests/test_gpu_merkle_update.py: the in-order walk -- what ordered leaf writes to a
Poseidon Merkle tree must return, restated in a few lines on the oracle's `poseidon` (oracle/fawkes_circuit.py, never the code under
test) -- and the cases of the device tests.  One oracle hash costs about a millisecond: a case keeps k * depth + 2^depth under 2500, the
pair hashes are memoised, and a case is computed once per session (`case`)."""
import functools
import random

import bn254_ref as ref
import fawkes_circuit as fc

R = ref.R
P3 = fc.PoseidonParams(3, 8, 53)
SPECIAL = (0, 1, R - 1)


@functools.lru_cache(maxsize=None)
def hash2(a, b):
    return fc.poseidon([a, b], P3)


def build_levels(leaves, depth):
    """levels[0] = the leaves zero-padded to 2^depth, ..., levels[depth] = [root]"""
    levels = [list(leaves) + [0] * ((1 << depth) - len(leaves))]
    assert len(levels[0]) == 1 << depth
    for _ in range(depth):
        lo = levels[-1]
        levels.append([hash2(lo[2 * i], lo[2 * i + 1]) for i in range(len(lo) // 2)])
    return levels


def walk(levels, indices, values):
    """the writes one after the other, each along its whole path; `levels` is updated in place -> (old_leaves, siblings, roots)"""
    depth = len(levels) - 1
    old, sibs, roots = [], [], []
    for idx, v in zip(indices, values):
        old.append(levels[0][idx])
        sib = []
        for l in range(depth):
            levels[l][idx >> l] = v
            s = levels[l][(idx >> l) ^ 1]
            sib.append(s)
            v = hash2(s, v) if (idx >> l) & 1 else hash2(v, s)
        levels[depth][0] = v
        sibs.append(sib)
        roots.append(v)
    return old, sibs, roots


class Case:
    """leaves, writes and what the walk says of them"""

    def __init__(self, depth, leaves, indices, values):
        self.depth, self.leaves, self.indices, self.values = depth, list(leaves), list(indices), list(values)
        levels = build_levels(self.leaves, depth)
        self.root_before = levels[depth][0]
        self.old, self.siblings, self.roots = walk(levels, self.indices, self.values)
        self.nodes = [x for lv in levels for x in lv]          # the final tree, in the device's layout
        self.n_leaves = max([len(self.leaves)] + [i + 1 for i in self.indices])


def values_for(k, rnd):
    """k field elements, 0, 1 and r - 1 among them wherever k allows"""
    v = [rnd.randrange(R) for _ in range(k)]
    for pos, s in zip(rnd.sample(range(k), min(k, 3)), SPECIAL):
        v[pos] = s
    return v


def leaves_for(n, rnd):
    return values_for(n, rnd)


@functools.lru_cache(maxsize=None)
def case(name, k=0):
    rnd = random.Random('%s/%d' % (name, k))
    if name == 'depth0':
        return Case(0, [rnd.randrange(R)], [0, 0, 0], [R - 1, 0, 1])
    if name in ('depth1_01', 'depth1_10'):              # the write-back hazard: the first write must see the OLD sibling
        return Case(1, [rnd.randrange(R), rnd.randrange(R)], [0, 1] if name == 'depth1_01' else [1, 0], [rnd.randrange(R), rnd.randrange(R)])
    if name == 'hot':                                   # depth 5, 20 leaves, a hot set of 8: runs collide on every level
        hot = rnd.sample(range(32), 8)
        return Case(5, leaves_for(20, rnd), [rnd.choice(hot) for _ in range(k)], values_for(k, rnd))
    if name == 'one_index':
        return Case(4, leaves_for(16, rnd), [11] * 64, values_for(64, rnd))
    if name == 'alternate':                             # each write's sibling is the previous write's value
        return Case(4, leaves_for(16, rnd), [6 + (j & 1) for j in range(64)], values_for(64, rnd))
    if name == 'edges':                                 # indices 0 and 2^depth - 1, and writes into the padding of 5 leaves (append)
        return Case(3, leaves_for(5, rnd), [0, 7, 5, 6, 0, 5, 7], values_for(7, rnd))
    raise KeyError(name)


def self_check():
    """the walk against a rebuild from the final leaves, and against the proof-root recomputation of the oracle"""
    c = case('hot', 65)
    final = list(c.leaves) + [0] * (32 - len(c.leaves))
    for i, v in zip(c.indices, c.values):
        final[i] = v
    assert c.nodes == [x for lv in build_levels(final, 5) for x in lv]
    before = [c.root_before] + c.roots[:-1]
    for j in (0, 1, 40, 64):
        path = [(c.indices[j] >> l) & 1 for l in range(5)]
        assert fc.poseidon_merkle_proof_root(c.old[j], c.siblings[j], path, P3) == before[j]
        assert fc.poseidon_merkle_proof_root(c.values[j], c.siblings[j], path, P3) == c.roots[j]
