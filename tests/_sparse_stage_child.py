"""Child of tests/test_gpu_sparse_merkle.py, run with FK_PROVE_SORTS_FIRST=1 (the schedule is chosen per process; tests/_stage_child.py
is the pattern): with two proofs submitted, `_wait` of the first queues the front of the second, whose a, b, c then sit in the staging
buffers.  Inside that window the sparse tree's `update` and `update_dev`, which sort in those buffers, are refused (code 1,
`early front`) and leave the tree alone; `proofs_dev`, `proofs` and `root`, which touch `misc` only, run and give what they gave
before; the waiting ticket yields its own proof; after the window `update` gives what it gave before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import fixtures as fx  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import api  # noqa: E402
from fawkes_crypto_amd import sparse_merkle as S  # noqa: E402
from helpers import r1cs_product, TOXIC  # noqa: E402
import check_cases as cc  # noqa: E402

ctx = fk.Context(0)
csr, z = cc.explicit_case(1000, seed=31)
prod = r1cs_product(csr)
wit = [z, cc.violate(csr, z, [5], seed=1)]
dk, vk = ctx.setup(prod, **{k: fx.mont_fr(v) for k, v in TOXIC.items()})
dr = ctx.load_r1cs(prod)
r, s = fx.mont_fr(0xA11CE), fx.mont_fr(0xB0B)
d_z = ctx.dev_alloc(z.nbytes)
direct = []
for w in wit:
    ctx.upload(d_z, w)
    direct.append(bytes(ctx.prove_witness_dev(dk, dr, d_z, r, s)))
assert len(set(direct)) == 2
pins = [ctx.host_alloc((len(z), 4)) for _ in range(2)]

# ---- everything the window's calls need, made before the window
p3 = api.PoseidonParams(3, 8, 53)
DEPTH = 32
FIRST = ([5, 1 << 31, (1 << 32) - 1], [11, 22, 33])


def fresh_tree():
    t = S.SparseMerkleTree(ctx, p3, DEPTH)
    t.update(*FIRST)
    return t


tree = fresh_tree()
ASK = np.array([5, 4, 77], np.uint64)
d_upd = {k: ctx.dev_alloc(b) for k, b in dict(idx=8, leaf=32, old=32, sib=32 * DEPTH, roots=32).items()}
ctx.upload(d_upd['idx'], np.array([4], np.uint64)); ctx.upload(d_upd['leaf'], api._fr_rows([44]))
d_ask, d_lv, d_sib = ctx.dev_alloc(8 * 3), ctx.dev_alloc(32 * 3), ctx.dev_alloc(32 * 3 * DEPTH)
ctx.upload(d_ask, ASK)


def state(t):
    return t.root, t.info(), [t.level_limbs(l)[1].tobytes() for l in range(DEPTH + 1)]


def update():
    t = fresh_tree()
    u = t.update([4, 5], [44, 55])
    out = (u.root_before, u.old_leaves, u.siblings, u.roots, t.root)
    t.free()
    return out


def update_dev():
    t = fresh_tree()
    try:
        t.update_dev(d_upd['idx'], d_upd['leaf'], 1, d_upd['old'], d_upd['sib'], d_upd['roots'])
        ctx.sync()
        return tuple(ctx.download(d_upd[k], 32 * (DEPTH if k == 'sib' else 1)).tobytes() for k in ('old', 'sib', 'roots')) + (t.root,)
    finally:
        t.free()


def proofs_dev():
    tree.proofs_dev(d_ask, 3, d_lv, d_sib)
    ctx.sync()
    return ctx.download(d_lv, 32 * 3).tobytes(), ctx.download(d_sib, 32 * 3 * DEPTH).tobytes()


CLAIMED = {'update': update, 'update_dev': update_dev}                                      # they sort in the staging buffers
ALLOWED = {'proofs_dev': proofs_dev, 'proofs': lambda: tree.proofs(ASK), 'root': lambda: tree.root}      # `misc` only: they run beside a front


def refused_on_the_resident_tree(name):
    """the same two calls on the tree made before the window: refused, or (no front) run on a copy's terms -- the tree is compared after"""
    if name == 'update':
        tree.update([4], [44])
    else:
        tree.update_dev(d_upd['idx'], d_upd['leaf'], 1, d_upd['old'], d_upd['sib'], d_upd['roots'])


before = {name: f() for name, f in {**CLAIMED, **ALLOWED}.items()}
assert before['proofs'][0] == [11, 0, 0] and before['update'][1] == [0, 11]
state0 = state(tree)

pins[0][:] = wit[0]; pins[1][:] = wit[1]
t_a = ctx.prove_witness_submit(dk, dr, pins[0], r, s)
t_b = ctx.prove_witness_submit(dk, dr, pins[1], r, s)
assert bytes(ctx.prove_witness_wait(t_a)) == direct[0]
refused = []
for name in CLAIMED:
    try:
        refused_on_the_resident_tree(name)
        refused.append(False)                       # no early front was queued (the schedule did not apply): nothing to refuse
    except fk.FkError as e:
        assert e.code == 1 and 'early front' in str(e), (name, str(e))
        refused.append(True)
assert all(refused) or not any(refused), dict(zip(CLAIMED, refused))
for name, f in ALLOWED.items():
    if all(refused):
        assert f() == before[name], name
assert bytes(ctx.prove_witness_wait(t_b)) == direct[1], 'the ticket behind the refused calls gave a wrong proof'
if all(refused):
    assert state(tree) == state0, 'a refused update wrote to the tree'
for name, f in {**CLAIMED, **ALLOWED}.items():
    if all(refused) or name in CLAIMED:
        assert f() == before[name], name
tree.free()
print('SPARSE STAGE ok refused=%s' % all(refused))
