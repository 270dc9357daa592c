"""Aggregated batch verification on the host (fk_verify_aggregate, csrc/verify_agg.hip through fawkes_crypto_amd/verify_agg.py; no GPU):
the verdict against the per-proof verifier, the report against Python integers over ref.G1, the cancellation attacks the weights exist
for, malformed proofs, the error codes and the fallback wrapper.  Every comparison is exact."""
import numpy as np
import pytest

import agg_cases as ac
import bn254_ref as ref


def _agg(vkb, inputs, proofs, weights=None):
    from fawkes_crypto_amd import verify_agg
    return verify_agg.verify_aggregate(None, vkb, inputs, proofs, weights)


_VERDICTS = {}


def _verify_each(vkb, inputs, proofs):
    """api.verify proof by proof (each distinct proof / inputs pair once per session)"""
    from fawkes_crypto_amd import api
    out = []
    for i in range(len(proofs)):
        k = (bytes(vkb), inputs[i].tobytes(), proofs[i].tobytes())
        if k not in _VERDICTS:
            _VERDICTS[k] = api.verify(vkb, inputs[i], proofs[i].tobytes())
        out.append(_VERDICTS[k])
    return out


def test_all_valid_and_the_report_in_python_integers(oracle):
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(5)
    assert len({p.tobytes() for p in proofs}) == 5
    w = ac.explicit_weights(5)
    accept, wf, rep = _agg(st.vkb, inputs, proofs, w)
    assert accept is True and wf.all()
    assert (rep.count, rep.n_wellformed, rep.equation_ok) == (5, 5, 1)
    sum_w, s_acc, s_c = ac.expected_sums(st, [st.z_in[1:]] * 5, proofs, w)
    assert tuple(rep.sum_w) == sum_w
    assert bytes(rep.s_acc) == s_acc
    assert bytes(rep.s_c) == s_c
    assert all(_verify_each(st.vkb, inputs, proofs))
    # weights drawn by the library: the same verdict, and another sum every time
    a1, _, r1 = _agg(st.vkb, inputs, proofs)
    a2, _, r2 = _agg(st.vkb, inputs, proofs)
    assert a1 and a2 and tuple(r1.sum_w) != tuple(r2.sum_w) and tuple(r1.sum_w) != sum_w


@pytest.mark.parametrize('kind', ac.KINDS)
def test_one_wrong_but_wellformed_proof_at_every_position(oracle, kind):
    st = ac.random_statement(oracle)
    w = ac.explicit_weights(5)
    for pos in range(5):
        inputs, proofs = st.batch(5)
        ac.make_wrong(inputs, proofs, pos, kind)
        accept, wf, rep = _agg(st.vkb, inputs, proofs, w)
        assert (rep.equation_ok, rep.n_wellformed, accept) == (0, 5, False), (kind, pos)
        each = _verify_each(st.vkb, inputs, proofs)
        assert each[pos] is False and accept == all(each)


def _cancellation(vkb, inputs, proofs):
    assert _verify_each(vkb, inputs, proofs) == [False, False]
    # THE ATTACK THE WEIGHTS EXIST FOR: each proof is wrong, but the errors of the two equations are opposite, so with equal weights
    # (or any weights the prover knows in advance) they cancel in the sum and the aggregated equation holds
    accept, wf, rep = _agg(vkb, inputs, proofs, [1, 1])
    assert wf.all() and rep.equation_ok == 1 and accept is True
    accept, wf, rep = _agg(vkb, inputs, proofs, [1, 2])
    assert wf.all() and rep.equation_ok == 0 and accept is False
    accept, wf, rep = _agg(vkb, inputs, proofs, None)             # secret weights: caught, except with probability ~2^-128
    assert wf.all() and rep.equation_ok == 0 and accept is False


def test_cancellation_on_the_c_side(oracle):
    _cancellation(*ac.swapped_c(oracle))


def test_cancellation_on_the_input_side(oracle):
    s0, s1 = ac.merkle_statements(oracle)
    assert _verify_each(s0.vkb, np.stack([s0.inputs, s1.inputs]), np.stack([s0.proof(0), s1.proof(0)])) == [True, True]
    _cancellation(*ac.swapped_inputs(oracle))


@pytest.mark.parametrize('kind', ac.MALFORMED)
def test_a_malformed_proof_is_flagged_and_left_out(oracle, kind):
    from fawkes_crypto_amd import api
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(4)
    ac.make_malformed(proofs, 2, kind)
    w = ac.explicit_weights(4)
    accept, wf, rep = _agg(st.vkb, inputs, proofs, w)            # returns (FK_OK): one bad submission does not fail the call
    assert list(wf) == [True, True, False, True]
    assert (rep.count, rep.n_wellformed, rep.equation_ok, accept) == (4, 3, 1, False)
    # its weight is in none of the three sums
    sum_w, s_acc, s_c = ac.expected_sums(st, [st.z_in[1:]] * 4, proofs, w, wellformed=wf)
    assert (tuple(rep.sum_w), bytes(rep.s_acc), bytes(rep.s_c)) == (sum_w, s_acc, s_c)
    assert b'first: proof 2' in api.load_library().fk_last_error(None)


def test_errors_and_edge_cases(oracle):
    import fawkes_crypto_amd as fk
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(3)
    with pytest.raises(fk.FkError) as e:
        _agg(st.vkb, inputs, proofs, [5, 0, 7])
    assert e.value.code == 1 and 'proof 1' in str(e.value)             # FK_ERR_BAD_ARG: a zero weight would drop the proof
    with pytest.raises(fk.FkError) as e:
        _agg(st.vkb, inputs[:, :1], proofs, [1, 2, 3])
    assert e.value.code == 6                                           # FK_ERR_KEY_MISMATCH
    with pytest.raises(fk.FkError) as e:
        _agg(st.vkb[:-1], inputs, proofs, [1, 2, 3])
    assert e.value.code == 7                                           # FK_ERR_FORMAT
    with pytest.raises(fk.FkError) as e:
        _agg(st.vkb[:100], inputs, proofs, [1, 2, 3])
    assert e.value.code == 7
    accept, wf, rep = _agg(st.vkb, inputs[:0], proofs[:0])
    assert accept is True and wf.size == 0 and (rep.count, rep.n_wellformed, rep.equation_ok) == (0, 0, 1)
    # a key with a coordinate that is no field element leaves no proof well-formed (the per-proof kernel rejects every proof under it)
    bad_vk = bytearray(st.vkb); bad_vk[0:32] = ref.Q.to_bytes(32, 'little')
    accept, wf, rep = _agg(bytes(bad_vk), inputs, proofs, [1, 2, 3])
    assert accept is False and not wf.any() and rep.n_wellformed == 0


def test_fallback_wrapper_equals_the_per_proof_verdicts(oracle):
    from fawkes_crypto_amd import verify_agg
    st = ac.random_statement(oracle)
    inputs, proofs = st.batch(12)
    ac.make_wrong(inputs, proofs, 1, 'c_other')
    ac.make_wrong(inputs, proofs, 4, 'input')
    ac.make_wrong(inputs, proofs, 7, 'a_identity')
    ac.make_malformed(proofs, 10, 'a_off_curve')
    want = _verify_each(st.vkb, inputs, proofs)
    assert want == [i not in (1, 4, 7, 10) for i in range(12)]
    got = verify_agg.verify_batch_aggregated(None, st.vkb, inputs, proofs)
    assert got.dtype == bool and list(got) == want
    # and an all-good batch comes back all True from the aggregate alone
    inputs, proofs = st.batch(12)
    assert verify_agg.verify_batch_aggregated(None, st.vkb, inputs, proofs).all()


def test_header_library_and_table_agree():
    """include/fawkes_hip_verify.h against the library and the module's ctypes table: every declared function is exported and listed,
    the struct has the C compiler's size"""
    import ctypes
    import os
    import re
    import fawkes_crypto_amd as fk
    from fawkes_crypto_amd import verify_agg
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fawkes_hip_verify.h')).read()
    declared = re.findall(r'^int (fk_\w+)\(', hdr, re.M)
    assert sorted(declared) == sorted(verify_agg.PROTOTYPES) == ['fk_verify_aggregate', 'fk_verify_aggregate_dev']
    lib = fk.load_library()
    assert all(hasattr(lib, s) for s in declared)
    assert not set(declared) & set(fk.EXPORTED_SYMBOLS)            # the pinned ABI of fawkes_hip.h is untouched
    assert ctypes.sizeof(verify_agg.AggReport) == 176 and verify_agg.AggReport.sum_w.offset == 16 and verify_agg.AggReport.s_c.offset == 112
