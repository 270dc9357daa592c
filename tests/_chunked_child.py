"""Child of tests/test_gpu_r1cs.py::test_prove_chunked_hand_over_under_either_schedule: the chunked hand-over of fk_prove_r1cs (the witness
goes up in pieces, ev_z is recorded behind the last piece and the prover is told so) under the schedule it was started with.  The schedule
is chosen per process (FK_PROVE_SORTS_FIRST, default: sorts-first from 2^25 on), hence the subprocess; without it the combination
chunked + sorts-first runs only at full size.  The system is the smallest explicit one that still gets row windows."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import bn254_ref as ref  # noqa: E402
import fixtures as fx  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
from helpers import r1cs_product, TOXIC  # noqa: E402
from test_gpu_r1cs import _local_system  # noqa: E402

gates, nin, naux = 70001, 3, 60000          # the loader plans windows from 16 * 4096 gates on; domain 2^17
nv = nin + naux
prod = r1cs_product(_local_system(99, [0, 1, 1, 1, 2, 3, 4, 9, 31, 32, 33, 70, 200], gates, nin, naux))
ctx = fk.Context(0)
dr = ctx.load_r1cs(prod)
w = dr.windows()
assert w is not None and len(w['need']) >= 2 and w['need'][0] < nv, w
key, _ = ctx.setup(prod, **{k: fx.mont_fr(v) for k, v in TOXIC.items()})
rnd = np.random.default_rng(5)
zs = []
for t in range(2):
    z = fx.co.limbs_arr([1] + [int(x) % ref.R for x in rnd.integers(1, 2**63, nv - 1).astype(object) * (2**190 + 12345 + t)])
    z[0] = fx.mont_fr(1)
    zs.append(z)
r, s = fx.mont_fr(0x1111), fx.mont_fr(0x2222)
d_z = ctx.dev_alloc(zs[0].nbytes)
ctx.upload(d_z, zs[1])
other = bytes(ctx.prove_witness_dev(key, dr, d_z, r, s))        # leaves ANOTHER witness's a, b, c in the staging buffers
got = bytes(ctx.prove_witness(key, dr, zs[0], r, s))             # chunked
ctx.upload(d_z, zs[0])
want = bytes(ctx.prove_witness_dev(key, dr, d_z, r, s))         # whole
assert got == want and got != other, 'the chunked proof differs from the whole-witness one'
assert bytes(ctx.prove_witness(key, dr, zs[1], r, s)) == other
# submit / wait / submit / wait over the same explicit system
pin = ctx.host_alloc((nv, 4))
for z, direct in ((zs[0], want), (zs[1], other)):
    pin[:] = z
    ticket = ctx.prove_witness_submit(key, dr, pin, r, s)
    assert bytes(ctx.prove_witness_wait(ticket)) == direct, 'a submitted proof differs from the direct one'
ctx.host_free(pin)
ctx.dev_free(d_z)
print('CHUNKED ok windows=%d' % len(w['need']))
