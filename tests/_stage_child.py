"""Child of tests/test_gpu_stage_claim.py, run with FK_PROVE_SORTS_FIRST=1 (the schedule is chosen per process): with two proofs submitted,
`_wait` of the first queues the front of the second -- its a, b, c then sit in the staging buffers and its sorts in the lanes.  Inside that
window every entry that borrows the staging buffers or the lanes is refused (code 1, `early front`) and leaves the front alone; the _dev
hashing and signature entries, which touch `misc` only, run and give what they gave before; the waiting ticket yields its own proof; after
the window every refused call gives what it gave before it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import fixtures as fx  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import api, merkle, verify_agg  # noqa: E402
from fawkes_crypto_amd import witness as W  # noqa: E402
from helpers import r1cs_product, TOXIC  # noqa: E402
import check_cases as cc  # noqa: E402
from test_gpu_witness import Gadget, _BUILD  # noqa: E402

ctx = fk.Context(0)
csr, z = cc.explicit_case(1000, seed=31)
prod = r1cs_product(csr)
wit = [z, cc.violate(csr, z, [5], seed=1), cc.violate(csr, z, [900], seed=2)]
dk, vk = ctx.setup(prod, **{k: fx.mont_fr(v) for k, v in TOXIC.items()})
dr = ctx.load_r1cs(prod)
r, s = fx.mont_fr(0xA11CE), fx.mont_fr(0xB0B)
d_z = ctx.dev_alloc(z.nbytes)
direct = []
for w in wit:
    ctx.upload(d_z, w)
    direct.append(bytes(ctx.prove_witness_dev(dk, dr, d_z, r, s)))
assert len(set(direct)) == 3
pins = [ctx.host_alloc((len(z), 4)) for _ in range(2)]

# ---- everything the window's calls need, made before the window
p3, p4 = api.PoseidonParams(3, 8, 53), api.PoseidonParams(4, 8, 54)
sk, msg = 0x1234567, 0x89abcdef
sig_s, sig_r, sig_a = (v[0] for v in ctx.eddsa_sign(p4, [sk], [msg]))
gadget = Gadget(*_BUILD['merkle2'])                     # the smallest traced circuit of tests/test_gpu_witness.py
prog = W.load(ctx, gadget.prog)
vkb = api.vk_to_borsh(vk)
inputs, proof0 = wit[0][1:prod.num_input].reshape(1, -1, 4), np.frombuffer(direct[0], np.uint8).reshape(1, -1)
tree = ctx.merkle_tree(p3, [11, 22])                    # depth 1
assert tree.depth == 1
nodes0 = tree.nodes().copy()
d_upd = {k: ctx.dev_alloc(32) for k in ('idx', 'leaf', 'old', 'sib', 'roots')}
ctx.upload(d_upd['idx'], np.array([1], np.uint64)); ctx.upload(d_upd['leaf'], api._fr_rows([33]))
one = fx.mont_fr(7).reshape(1, 4)
two = np.stack([fx.mont_fr(3), fx.mont_fr(5)])
squares = ctx.fr_mul_batch(two, two)
d_pt, d_sc = ctx.dev_alloc(64), ctx.dev_alloc(32)
ctx.gen_points_g1_dev(d_pt, 1, 99); ctx.upload(d_sc, one); ctx.sync()
point = ctx.download(d_pt, 64)
d_hash_in, d_hash_out = ctx.dev_alloc(64), ctx.dev_alloc(32)
ctx.upload(d_hash_in, api._fr_rows([1, 2]))
d_sig = [ctx.dev_alloc(32) for _ in range(4)] + [ctx.dev_alloc(1)]
for d, arr in zip(d_sig, (api._u256_rows([sig_s]), api._fr_rows([sig_r]), api._fr_rows([sig_a]), api._fr_rows([msg]))):
    ctx.upload(d, arr)


def restore_tree():
    ctx.upload(tree.d_nodes, nodes0)
    tree.n_leaves, tree._root = 2, None


def merkle_update():
    restore_tree()
    u = merkle.update(tree, p3, [0], [44])
    return u.root_before, u.old_leaves, u.siblings, u.roots, tree.nodes().tobytes()


def merkle_update_dev():
    restore_tree()
    merkle.update_dev(ctx, p3, tree.d_nodes, 1, d_upd['idx'], d_upd['leaf'], 1, d_upd['old'], d_upd['sib'], d_upd['roots'])
    ctx.sync()
    return tuple(ctx.download(d_upd[k], 32).tobytes() for k in ('old', 'sib', 'roots')) + (tree.nodes().tobytes(),)


def hash_dev():
    ctx.poseidon_dev(p3, d_hash_in, 2, 1, d_hash_out)
    ctx.sync()
    return ctx.download(d_hash_out, 32).tobytes()


def eddsa_verify_dev():
    ctx.eddsa_verify_dev(p4, d_sig[0], d_sig[1], d_sig[2], d_sig[3], 1, d_sig[4])
    ctx.sync()
    return ctx.download(d_sig[4], 1).tolist()


def aggregate():
    accept, wellformed, _ = verify_agg.verify_aggregate(ctx, vkb, inputs, proof0)       # (the report holds the drawn weights)
    return accept, wellformed.tolist()


CLAIMED = {      # every entry that borrows the staging buffers or the lanes, at its smallest shape
    'poseidon': lambda: ctx.poseidon(p3, [(1, 2)]),
    'poseidon_sponge': lambda: ctx.poseidon_sponge(p3, [(5,)]),
    'merkle_root': lambda: ctx.merkle_root(p3, [11, 22]),
    'merkle_proof_roots': lambda: ctx.merkle_proof_roots(p3, [11], [22], [0], 1),
    'jubjub_mul': lambda: ctx.jubjub_mul(None, [5]),
    'jubjub_decompress': lambda: ctx.jubjub_decompress([sig_a]),
    'eddsa_sign': lambda: ctx.eddsa_sign(p4, [sk], [msg]),
    'eddsa_verify': lambda: ctx.eddsa_verify(p4, [sig_s], [sig_r], [sig_a], [msg]),
    'witness.generate': lambda: W.generate(ctx, prog, [gadget.given[0]]).tobytes(),
    'verify_batch': lambda: api.verify_batch(ctx, vkb, inputs, proof0).tolist(),
    'verify_aggregate_dev': aggregate,
    'merkle.update': merkle_update,
    'merkle.update_dev': merkle_update_dev,
    'fr_mul_batch': lambda: ctx.fr_mul_batch(one, one).tobytes(),
    'quotient_h': lambda: ctx.quotient_h(two, two, squares).tobytes(),
    'msm_g1': lambda: ctx.msm_g1(point, one).tobytes(),
    'msm_g1_dev': lambda: ctx.msm_g1_dev(d_pt, d_sc, 1).tobytes(),
}
ALLOWED = {'poseidon_dev': hash_dev, 'eddsa_verify_dev': eddsa_verify_dev}      # `misc` only: they run beside a front

before = {name: f() for name, f in {**CLAIMED, **ALLOWED}.items()}
assert before['eddsa_verify'] == [True] and before['eddsa_verify_dev'] == [1] and before['verify_batch'] == [True] and before['verify_aggregate_dev'] == (True, [True])
restore_tree()

pins[0][:] = wit[0]; pins[1][:] = wit[1]
t_a = ctx.prove_witness_submit(dk, dr, pins[0], r, s)
t_b = ctx.prove_witness_submit(dk, dr, pins[1], r, s)
assert bytes(ctx.prove_witness_wait(t_a)) == direct[0]
refused = []
for name, f in CLAIMED.items():
    try:
        f()
        refused.append(False)                       # no early front was queued (the schedule did not apply): nothing to refuse
    except fk.FkError as e:
        assert e.code == 1 and 'early front' in str(e), (name, str(e))
        refused.append(True)
assert all(refused) or not any(refused), dict(zip(CLAIMED, refused))
if all(refused):
    assert tree.nodes().tobytes() == nodes0.tobytes(), 'a refused update wrote to the tree'
for name, f in ALLOWED.items():
    assert f() == before[name], name
assert bytes(ctx.prove_witness_wait(t_b)) == direct[1], 'the ticket behind the refused calls gave a wrong proof'
for name, f in {**CLAIMED, **ALLOWED}.items():
    assert f() == before[name], name
ctx.upload(d_z, wit[2])
assert bytes(ctx.prove_witness_dev(dk, dr, d_z, r, s)) == direct[2]
print('STAGE ok refused=%s' % all(refused))
