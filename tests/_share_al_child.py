"""Child of tests/test_gpu_share_al_sort.py: proves every case of tests/share_al_cases.py under the environment it was started with (the
switches are read once per process) and prints the proof bytes with what fk_key_a_pad_info says about the key afterwards.  The keys
come from the parent (the oracle's, one .npz per system); systems and witnesses are rebuilt here from the same seeds.
argv: the directory with the .npz files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import fixtures as fx  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
import share_al_cases as sc  # noqa: E402
from helpers import r1cs_product  # noqa: E402

kdir = sys.argv[1]
ctx = fk.Context(0)
cases, tile = sc.case_list()
r, s = fx.mont_fr(sc.R_S[0]), fx.mont_fr(sc.R_S[1])


def say(tag, **kw):
    print('RESULT ' + json.dumps(dict(tag=tag, **kw)), flush=True)


def load(n, dname, variant='plain'):
    arrays = dict(np.load(os.path.join(kdir, '%d-%s.npz' % (n, dname))))
    if variant == 'repeats':
        arrays = sc.with_repeats_and_infinities(arrays)
    csr = sc.system(n, sc.density(dname, n, tile), seed=n)
    prod = r1cs_product(csr)
    return csr, ctx.load_key(fk.Parameters(arrays, prod)), ctx.load_r1cs(prod)


def pad_info(key):
    """fk_key_a_pad_info (include/fawkes_hip_inspect.h: test-only, called through ctypes directly)"""
    import ctypes as C
    lib = fk.load_library()
    lib.fk_key_a_pad_info.restype, lib.fk_key_a_pad_info.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 6)()
    assert lib.fk_key_a_pad_info(key.handle, out) == 0
    return dict(in_place=bool(out[0]), points=int(out[1]), levels=int(out[2]), refused=bool(out[3]), arrays=int(out[0]), queries=int(out[4]), bytes=int(out[5]))


def hexproof(p):
    return bytes(p).hex()


# ---- every case, a fresh key each (the first proof with a key builds the padded array)
for c in cases:
    n, dname, wname, variant = c
    csr, key, dr = load(n, dname, variant)
    z = sc.witness(wname, n, seed=n + 1)
    p1 = hexproof(ctx.prove_witness(key, dr, z, r, s))
    p2 = hexproof(ctx.prove_witness(key, dr, z, r, s))         # warm: the array is in place, the lanes hold their buffers
    say('case', id=sc.case_id(c), proof=p1, again=p2, pad=pad_info(key), levels=key.precomputed())
    dr.free(); key.free()

# ---- one key, two systems with different A queries, in one context: the fingerprint and the rebuild
n = sc.sizes()[0][1]
csr1, key, dr1 = load(n, 'alternating')
prod2 = r1cs_product(sc.system(n, sc.second_density(n, tile), seed=n + 7))
dr2 = ctx.load_r1cs(prod2)
z1, z2 = sc.witness('random', n, seed=n + 1), sc.witness('random', n, seed=n + 2)
seq = []
for dr, z in ((dr1, z1), (dr2, z1), (dr2, z2), (dr1, z2), (dr1, z1)):
    seq.append(hexproof(ctx.prove_witness(key, dr, z, r, s)))
say('two_systems', proofs=seq, pad=pad_info(key))

# ---- the two-slot pipeline with different witnesses in flight: the next proof's early front sorts on L's lane while this proof's A may
# still read the sort it borrowed
nv = z1.shape[0]
pins = [ctx.host_alloc((nv, 4)) for _ in range(2)]
wit = [z1, z2, sc.witness('ones', n, seed=0), sc.witness('zeros', n, seed=0)]
direct = [hexproof(ctx.prove_witness(key, dr1, z, r, s)) for z in wit]
order = [0, 1, 2, 3, 1, 0, 3, 2, 0]
got = []
pins[0][:] = wit[order[0]]
ticket = ctx.prove_witness_submit(key, dr1, pins[0], r, s)
for k in range(len(order)):
    nxt = None
    if k + 1 < len(order):
        pins[(k + 1) & 1][:] = wit[order[k + 1]]
        nxt = ctx.prove_witness_submit(key, dr1, pins[(k + 1) & 1], r, s)
    got.append(hexproof(ctx.prove_witness_wait(ticket)))
    ticket = nxt
say('pipeline', direct=direct, order=order, got=got, pad=pad_info(key))

# ---- a foreign proof while A's borrowed sort is still pending: wait(A) queues ticket B's early front (A's aux part begun, its accumulation
# deferred), a foreign proof finds the front outstanding and is refused, and ticket B still gives its own proof
d_zf = ctx.dev_alloc(nv * 32)
ctx.upload(d_zf, wit[2])
pins[0][:] = wit[0]; pins[1][:] = wit[1]
t_a = ctx.prove_witness_submit(key, dr1, pins[0], r, s)
t_b = ctx.prove_witness_submit(key, dr1, pins[1], r, s)
first = hexproof(ctx.prove_witness_wait(t_a))
try:
    foreign = hexproof(ctx.prove_witness_dev(key, dr1, d_zf, r, s))
    refused = None
except fk.FkError as e:
    foreign, refused = None, [e.code, str(e)]
second = hexproof(ctx.prove_witness_wait(t_b))
third = hexproof(ctx.prove_witness_dev(key, dr1, d_zf, r, s))
ctx.dev_free(d_zf)
say('abandon', first=first, foreign=foreign, refused=refused, second=second, third=third)

# ---- after fk_trim, and after a call that fails inside the witness multiplications' front (a system whose A query the key does not fit)
ctx.trim()
after_trim = hexproof(ctx.prove_witness(key, dr1, z1, r, s))
csr_all = sc.system(n, sc.density('all', n, tile), seed=n)
dr_all = ctx.load_r1cs(r1cs_product(csr_all))
try:
    ctx.prove_witness(key, dr_all, z1, r, s)
    err = None
except fk.FkError as e:
    err = [e.code, str(e)]
after_error = hexproof(ctx.prove_witness(key, dr1, z1, r, s))
say('recovery', want=direct[0], after_trim=after_trim, error=err, after_error=after_error, pad=pad_info(key))

# ---- the fallback: the two halves of a key split by points keep A's own sort and fold to the unsharded proof
import c_oracle as co  # noqa: E402
a, b, c_, aa, bi, ba = co.synthesize(csr1, z1)
m = int(np.load(os.path.join(kdir, '%d-alternating.npz' % n))['m'])
d = {k: ctx.dev_alloc(m * 32) for k in 'abch'}
d_z = ctx.dev_alloc(z1.nbytes)
for k_, v in (('a', a), ('b', b), ('c', c_)):
    ctx.upload(d[k_], np.ascontiguousarray(np.concatenate([v, np.zeros((m - v.shape[0], 4), np.uint64)])))
ctx.upload(d_z, z1)
ctx.quotient_h_dev(d['a'], d['b'], d['c'], a.shape[0], d['h'])
params = fk.Parameters(dict(np.load(os.path.join(kdir, '%d-alternating.npz' % n))), r1cs_product(csr1))
parts, pads = [], []
for g in range(2):
    sk = ctx.load_key(params, shard_index=g, shard_count=2)
    h_lo = sk.shard_info()['h'][0]
    parts.append(ctx.prove_msms_hz_r1cs_dev(sk, dr1, d['h'] + h_lo * 32, d_z))
    pads.append(pad_info(sk))
    sk.free()
folded = hexproof(ctx.prove_assemble(key, np.stack(parts), r, s))
say('sharded', want=direct[0], folded=folded, pads=pads)
print('DONE', flush=True)
