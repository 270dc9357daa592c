"""Shared by tests/test_sparse_merkle_host.py and tests/test_gpu_sparse_merkle.py: the in-order walk of tests/merkle_cases.py restated
over dicts -- a level holds the nodes some write has passed through, every other node of level l is zero[l], zero[0] = 0,
zero[l + 1] = H(zero[l], zero[l]) -- on the same memoised oracle hash (merkle_cases.hash2, never the code under test), and the deep
cases of the device tests.  One oracle hash costs about a millisecond: a case keeps writes * depth + depth under 2500 and is computed
once per session."""
import functools
import random

import merkle_cases as mc

R = mc.R


def defaults(depth):
    """zero[0 .. depth]"""
    z = [0]
    for _ in range(depth):
        z.append(mc.hash2(z[-1], z[-1]))
    return z


class SparseWalk:
    """levels[l]: {node index: value} of the nodes written so far, l = 0 .. depth (levels[depth] = {0: root} once anything was written)"""

    def __init__(self, depth):
        self.depth, self.zero = depth, defaults(depth)
        self.levels = [{} for _ in range(depth + 1)]

    def get(self, l, node):
        return self.levels[l].get(node, self.zero[l])

    @property
    def root(self):
        return self.get(self.depth, 0)

    def walk(self, indices, values):
        """the writes one after the other, each along its whole path -> (old_leaves, siblings, roots)"""
        old, sibs, roots = [], [], []
        for idx, v in zip(indices, values):
            assert 0 <= idx < 1 << self.depth
            old.append(self.get(0, idx))
            sib = []
            for l in range(self.depth):
                node = idx >> l
                self.levels[l][node] = v
                s = self.get(l, node ^ 1)
                sib.append(s)
                v = mc.hash2(s, v) if node & 1 else mc.hash2(v, s)
            self.levels[self.depth][0] = v
            sibs.append(sib)
            roots.append(v)
        return old, sibs, roots

    def proof(self, idx):
        """(leaf, siblings) of any index, written or not"""
        return self.get(0, idx), [self.get(l, (idx >> l) ^ 1) for l in range(self.depth)]


class SparseCase:
    """initial writes (applied first, as ordinary writes), the writes under test, and what the walk says of them"""

    def __init__(self, depth, initial, indices, values):
        self.depth, self.initial, self.indices, self.values = depth, list(initial), list(indices), list(values)
        self.tree = SparseWalk(depth)
        self.tree.walk([i for i, _ in self.initial], [v for _, v in self.initial])
        self.root_before = self.tree.root
        self.old, self.siblings, self.roots = self.tree.walk(self.indices, self.values)
        self.levels = self.tree.levels          # the final state


def from_dense(c):
    """a case of merkle_cases as a sparse one: its initial leaves become the first writes"""
    return SparseCase(c.depth, list(enumerate(c.leaves)), c.indices, c.values)


@functools.lru_cache(maxsize=None)
def case(name):
    rnd = random.Random('sparse/' + name)
    if name == 'deep32':        # 40 writes: both ends, a sibling pair, one index three times, pairs equal in all but the top / the bottom bit
        top = 1 << 31
        a, b, c = rnd.randrange(top), rnd.randrange(top) & ~1, rnd.randrange(1 << 32)
        fixed = [0, (1 << 32) - 1, 0x12345678, 0x12345679, c, c, c, a, a | top, b, b | 1]
        initial = [(i, rnd.randrange(1, R)) for i in (0, 0x12345679, a | top, rnd.randrange(1 << 32), rnd.randrange(1 << 32))]
        indices = fixed + [rnd.randrange(1 << 32) for _ in range(40 - len(fixed))]
        rnd.shuffle(indices)
        return SparseCase(32, initial, indices, mc.values_for(40, rnd))
    if name == 'deep63':        # 16 writes, keys that need 64 bits: indices at and above 2^62, 2^63 - 1 among them
        hi = 1 << 62
        fixed = [(1 << 63) - 1, (1 << 63) - 2, hi, hi | 1, 0, hi - 1, hi + rnd.randrange(hi), (1 << 63) - 1]
        indices = fixed + [rnd.randrange(1 << 63) for _ in range(16 - len(fixed))]
        rnd.shuffle(indices)
        initial = [((1 << 63) - 1, rnd.randrange(1, R)), (hi, rnd.randrange(1, R))]
        return SparseCase(63, initial, indices, mc.values_for(16, rnd))
    raise KeyError(name)
