"""Aggregated batch verification on the GPU (fk_verify_aggregate_dev: agg_prepare_kernel, agg_miller_kernel, f12_level_kernel,
g1_level_kernel of csrc/verify_agg.hip) against the host entry, which runs the same templates on the CPU and is itself checked against
Python integers and the per-proof verifier in test_verify_aggregate_host.py.  Sizes: one lane, one pair, a wave less one, a full wave, a
wave and one, an odd tail on two levels (67), a third wave (130).  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import agg_cases as ac
import fixtures as fx

pytestmark = pytest.mark.gpu


def _both(ctx, vkb, inputs, proofs, weights):
    from fawkes_crypto_amd import verify_agg
    return verify_agg.verify_aggregate(ctx, vkb, inputs, proofs, weights), verify_agg.verify_aggregate(None, vkb, inputs, proofs, weights)


def _raw(rep):
    return ctypes.string_at(ctypes.addressof(rep), ctypes.sizeof(rep))


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 67, 130])
def test_device_equals_host_on_valid_batches(ctx, oracle, n):
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(n)
    (acc_d, wf_d, rep_d), (acc_h, wf_h, rep_h) = _both(ctx, st.vkb, inputs, proofs, ac.explicit_weights(n))
    assert acc_h is True and wf_h.all() and rep_h.n_wellformed == n
    assert acc_d == acc_h and np.array_equal(wf_d, wf_h)
    assert _raw(rep_d) == _raw(rep_h)                  # every byte: the counts, the verdict, sum_w, S_acc, S_C


@pytest.mark.parametrize('pos, kind', [(0, 'c_other'), (1, 'a_other'), (63, 'input'), (64, 'a_identity'), (65, 'c_other'), (66, 'a_other')])
def test_one_wrong_proof_in_67_is_caught_wherever_it_sits(ctx, oracle, pos, kind):
    """a lane or a level tail that is dropped would let the batch through"""
    from fawkes_crypto_amd import verify_agg
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(67)
    ac.make_wrong(inputs, proofs, pos, kind)
    accept, wf, rep = verify_agg.verify_aggregate(ctx, st.vkb, inputs, proofs, ac.explicit_weights(67))
    assert wf.all() and (rep.n_wellformed, rep.equation_ok, accept) == (67, 0, False)


@pytest.mark.parametrize('case', ['c', 'inputs'])
def test_cancellation_on_the_device(ctx, oracle, case):
    """the outcomes of the host file: equal (known) weights let two wrong proofs cancel, unequal or secret ones do not"""
    vkb, inputs, proofs = ac.swapped_c(oracle) if case == 'c' else ac.swapped_inputs(oracle)
    for weights, want in (([1, 1], 1), ([1, 2], 0)):
        (acc_d, wf_d, rep_d), (acc_h, wf_h, rep_h) = _both(ctx, vkb, inputs, proofs, weights)
        assert wf_d.all() and rep_d.equation_ok == want and acc_d is bool(want)
        assert _raw(rep_d) == _raw(rep_h)
    from fawkes_crypto_amd import verify_agg
    accept, wf, rep = verify_agg.verify_aggregate(ctx, vkb, inputs, proofs, None)
    assert wf.all() and rep.equation_ok == 0 and accept is False


@pytest.mark.parametrize('kind', ac.MALFORMED)
def test_malformed_proofs_on_the_device(ctx, oracle, kind):
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(4)
    ac.make_malformed(proofs, 2, kind)
    (acc_d, wf_d, rep_d), (acc_h, wf_h, rep_h) = _both(ctx, st.vkb, inputs, proofs, ac.explicit_weights(4))
    assert list(wf_d) == [True, True, False, True]
    assert (rep_d.n_wellformed, rep_d.equation_ok, acc_d) == (3, 1, False)
    assert _raw(rep_d) == _raw(rep_h)
    assert b'first: proof 2' in ctx.lib.fk_last_error(ctx.handle)


def test_fallback_wrapper_on_the_mix_of_the_batch_verifier_test(ctx, oracle):
    """the 70 proofs of test_batch_verifier_on_the_gpu, every third one tampered with; then with the proof that does not decode"""
    from fawkes_crypto_amd import api, verify_agg
    st = ac.random_statement(oracle)
    n = 70
    proofs = np.tile(st.proof(0), (n, 1))
    inputs = np.tile(st.inputs, (n, 1, 1))
    want = np.ones(n, bool)
    for i in range(0, n, 3):
        if i % 2:
            proofs[i, 200] ^= 4
        else:
            inputs[i, 1] = fx.mont_fr(i + 5)
        want[i] = False
    got = verify_agg.verify_batch_aggregated(ctx, st.vkb, inputs, proofs)
    assert np.array_equal(got, want) and np.array_equal(got, api.verify_batch(ctx, st.vkb, inputs, proofs))
    proofs[7, 0:32] = 0xff
    want[7] = False
    got = verify_agg.verify_batch_aggregated(ctx, st.vkb, inputs, proofs)
    assert np.array_equal(got, want) and np.array_equal(got, api.verify_batch(ctx, st.vkb, inputs, proofs))
    # all good: the aggregate alone answers
    inputs, proofs = st.batch(n)
    assert verify_agg.verify_batch_aggregated(ctx, st.vkb, inputs, proofs).all()


def test_nothing_is_left_outstanding_on_the_context(ctx, oracle):
    """the call borrows the context's scratch and stream: a proof and a per-proof batch verification on the same context afterwards"""
    import c_oracle as co
    import bn254_ref as ref
    import fawkes_crypto_amd as fk
    from fawkes_crypto_amd import api, verify_agg
    from helpers import params_from_oracle_key, r1cs_product, TOXIC
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(65)
    assert verify_agg.verify_aggregate(ctx, st.vkb, inputs, proofs)[0] is True
    cs, z_in, z_aux = ref.random_r1cs(2026, 60, 2, 70)
    csr = fx.r1cs_to_csr(cs)
    key = co.setup(csr, **TOXIC)
    params = params_from_oracle_key(key, r1cs_product(csr))
    dk = ctx.load_key(params)
    z = fx.witness_mont(z_in, z_aux)
    r, s = fx.mont_fr(0x5eed), fx.mont_fr(0xfeed)
    _, proof = fk.prove_with_rs(ctx, params, dk, z[:2], z[2:], r, s)
    a, b, c, aa, bi, ba = co.synthesize(csr, z)
    assert proof.to_bytes() == co.prove(key, a, b, c, z, aa, bi, ba, r, s).tobytes()
    assert api.verify_batch(ctx, st.vkb, inputs, proofs).all()
    assert verify_agg.verify_aggregate(ctx, st.vkb, inputs, proofs)[0] is True
