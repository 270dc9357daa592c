"""Child of tests/test_gpu_r1cs_check.py::test_an_outstanding_early_front_is_refused, run with FK_PROVE_SORTS_FIRST=1 (the schedule is
chosen per process): with two proofs submitted, `_wait` of the first queues the front of the second -- its a, b, c then sit in the
staging buffers.  A check that would overwrite them is refused and leaves the front alone; the checked proof, which does not join the
pipeline, is refused the way a foreign fk_prove_r1cs_dev is (the front is dropped); the waiting ticket yields its own proof either way."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import fixtures as fx  # noqa: E402
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import check as K  # noqa: E402
from helpers import r1cs_product, TOXIC  # noqa: E402
import check_cases as cc  # noqa: E402

ctx = fk.Context(0)
csr, z = cc.explicit_case(1000, seed=31)
prod = r1cs_product(csr)
wit = [z, cc.violate(csr, z, [5], seed=1), cc.violate(csr, z, [900], seed=2)]
dk, _ = ctx.setup(prod, **{k: fx.mont_fr(v) for k, v in TOXIC.items()})
dr = ctx.load_r1cs(prod)
r, s = fx.mont_fr(0xA11CE), fx.mont_fr(0xB0B)
d_z = ctx.dev_alloc(z.nbytes)
direct = []
for w in wit:
    ctx.upload(d_z, w)
    direct.append(bytes(ctx.prove_witness_dev(dk, dr, d_z, r, s)))
assert len(set(direct)) == 3
pins = [ctx.host_alloc((len(z), 4)) for _ in range(2)]
refused = []
for attempt in ('check', 'prove'):
    pins[0][:] = wit[0]; pins[1][:] = wit[1]
    t_a = ctx.prove_witness_submit(dk, dr, pins[0], r, s)
    t_b = ctx.prove_witness_submit(dk, dr, pins[1], r, s)
    assert bytes(ctx.prove_witness_wait(t_a)) == direct[0]
    ctx.upload(d_z, wit[2])
    try:
        if attempt == 'check':
            K.check_witness(ctx, dr, d_z)
        else:
            K.prove_checked(ctx, dk, dr, d_z, r, s)
        refused.append(False)                       # no early front was queued (the schedule did not apply): nothing to refuse
    except fk.FkError as e:
        assert e.code == 1 and 'early front' in str(e), str(e)
        refused.append(True)
    assert bytes(ctx.prove_witness_wait(t_b)) == direct[1], 'the ticket behind a refused call gave a wrong proof'
    proof, rep = K.prove_checked(ctx, dk, dr, d_z, r, s)
    assert bytes(proof) == direct[2] and rep.bad_rows().tolist() == cc.Want(csr, wit[2]).bad and 900 in rep.bad_rows().tolist()
    assert K.check_witness(ctx, dr, d_z).n_bad == rep.n_bad
ctx.dev_free(d_z)
print('CHECK ok early_front_refused=%s' % all(refused))
