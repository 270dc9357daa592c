"""Fixtures of the aggregated-verifier tests (test_verify_aggregate_host.py, test_gpu_verify_aggregate.py): batches of distinct valid
proofs under one key, the ways of making a proof wrong without taking it off its curves, and the malformed proofs.  Everything is built
with the oracle, once per session, and handed out as copies."""
import random

import numpy as np

import bn254_ref as ref
import fixtures as fx
from helpers import TOXIC

_CACHE = {}

KINDS = ('c_other', 'a_other', 'input', 'a_identity')      # wrong but well-formed: every point stays on its curve


def vk_of(key):
    return dict(alpha_g1=key.alpha_g1, beta_g2=key.beta_g2, gamma_g2=key.gamma_g2, delta_g2=key.delta_g2, ic=np.array(key.ic))


class Statement:
    """one constraint system with its key and one witness; proof(i) is the i-th distinct valid proof of it (its own r, s)"""

    def __init__(self, oracle, csr, z_in, z_aux, key=None):
        from fawkes_crypto_amd import api
        self.oracle, self.csr, self.z_in = oracle, csr, list(z_in)
        self.key = key if key is not None else oracle.setup(csr, **TOXIC)
        self.vkb = api.vk_to_borsh(vk_of(self.key))
        self.z = fx.witness_mont(z_in, z_aux)
        self.syn = oracle.synthesize(csr, self.z)
        self.inputs = self.z[1:len(z_in)].copy()            # (n_inputs, 4) Montgomery
        self._proofs = {}

    def proof(self, i):
        if i not in self._proofs:
            a, b, c, aa, bi, ba = self.syn
            self._proofs[i] = self.oracle.prove(self.key, a, b, c, self.z, aa, bi, ba, fx.mont_fr(7 * i + 1001), fx.mont_fr(11 * i + 2002)).copy()
        return self._proofs[i]

    def batch(self, n):
        """(inputs (n, n_inputs, 4), proofs (n, 256)): n distinct valid proofs"""
        return np.tile(self.inputs, (n, 1, 1)), np.stack([self.proof(i) for i in range(n)])


def random_statement(oracle):
    """the instance of test_batch_verifier_on_the_gpu: 60 gates, two public inputs"""
    if 'random' not in _CACHE:
        cs, z_in, z_aux = ref.random_r1cs(9, 60, 3, 70)
        _CACHE['random'] = Statement(oracle, fx.r1cs_to_csr(cs), z_in, z_aux)
    return _CACHE['random']


def merkle_statements(oracle):
    """two statements of one circuit under one key: the depth-2 Poseidon Merkle proof of two different leaves"""
    if 'merkle' not in _CACHE:
        import fawkes_circuit as fc
        rnd = random.Random(2)
        sib, path = [rnd.randrange(ref.R) for _ in range(2)], [1, 0]
        cs = [fc.poseidon_merkle_circuit(leaf, sib, path, depth=2)[0] for leaf in (rnd.randrange(ref.R), rnd.randrange(ref.R))]
        assert cs[0].gates == cs[1].gates and cs[0].z_in != cs[1].z_in
        s0 = Statement(oracle, fx.r1cs_to_csr(cs[0].r1cs()), cs[0].z_in, cs[0].z_aux)
        s1 = Statement(oracle, s0.csr, cs[1].z_in, cs[1].z_aux, key=s0.key)
        _CACHE['merkle'] = (s0, s1)
    return _CACHE['merkle']


def make_wrong(inputs, proofs, pos, kind):
    """in place: proof `pos` of the batch becomes wrong but stays well-formed"""
    other = (pos + 1) % len(proofs)
    if kind == 'c_other':
        proofs[pos, 192:256] = proofs[other, 192:256]
    elif kind == 'a_other':
        proofs[pos, 0:64] = proofs[other, 0:64]
    elif kind == 'input':
        inputs[pos, 0] = fx.mont_fr(12345 + pos)
    elif kind == 'a_identity':
        proofs[pos, 0:64] = 0
    else:
        raise ValueError(kind)


def point_outside_the_subgroup():
    """a point ON the twist that is not in the order-r subgroup (the construction of test_host_verifier_rejects_points_outside_the_groups)"""
    if 'g2_bad' in _CACHE:
        return _CACHE['g2_bad']
    F2, b2 = ref.F2, ref.G2.b

    def fq_sqrt(v):
        y = pow(v, (ref.Q + 1) // 4, ref.Q)
        return y if y * y % ref.Q == v % ref.Q else None

    def fq2_sqrt(a0, a1):
        alpha = fq_sqrt((a0 * a0 + a1 * a1) % ref.Q)
        if alpha is None:
            return None
        for d in ((a0 + alpha) * pow(2, -1, ref.Q) % ref.Q, (a0 - alpha) * pow(2, -1, ref.Q) % ref.Q):
            x0 = fq_sqrt(d)
            if x0:
                return x0, a1 * pow(2 * x0, -1, ref.Q) % ref.Q
        return None
    x = (11, 3)
    while True:
        rhs = F2.add(F2.mul(F2.sqr(x), x), b2)
        y = fq2_sqrt(*rhs)
        if y is not None and F2.sqr(y) == rhs:
            break
        x = (x[0] + 1, x[1])
    assert ref.G2.on_curve((x, y)) and ref.G2.mul((x, y), ref.R) is not None
    _CACHE['g2_bad'] = (x, y)
    return x, y


MALFORMED = ('coordinate_q', 'a_off_curve', 'b_outside_subgroup')


def make_malformed(proofs, pos, kind):
    """in place: proof `pos` stops being well-formed"""
    A, B, C = ref.proof_from_borsh(proofs[pos].tobytes())
    if kind == 'coordinate_q':
        proofs[pos, 0:32] = np.frombuffer(ref.Q.to_bytes(32, 'little'), np.uint8)
    elif kind == 'a_off_curve':
        proofs[pos] = np.frombuffer(ref.proof_borsh((A[0], (A[1] + 1) % ref.Q), B, C), np.uint8)
    elif kind == 'b_outside_subgroup':
        proofs[pos] = np.frombuffer(ref.proof_borsh(A, point_outside_the_subgroup(), C), np.uint8)
    else:
        raise ValueError(kind)


def swapped_c(oracle):
    """two valid proofs of one statement with their C swapped: each is wrong, the SUM of the two equations still holds"""
    inputs, proofs = random_statement(oracle).batch(2)
    proofs[[0, 1], 192:256] = proofs[[1, 0], 192:256]
    return random_statement(oracle).vkb, inputs, proofs


def swapped_inputs(oracle):
    """the proofs of the two Merkle statements, each presented with the other's root"""
    s0, s1 = merkle_statements(oracle)
    inputs = np.stack([s1.inputs, s0.inputs])
    proofs = np.stack([s0.proof(0), s1.proof(0)])
    return s0.vkb, inputs, proofs


def expected_sums(stmt, inputs_ints, proofs, weights, wellformed=None):
    """(sum_w limbs, s_acc raw bytes, s_c raw bytes) in Python integers over ref.G1: what the report must hold exactly"""
    G1 = ref.G1
    n = len(proofs)
    live = [i for i in range(n) if wellformed is None or wellformed[i]]
    sw = sum(weights[i] for i in live) % ref.R
    ic = [ref.g1_from_raw_le(bytes(r)) for r in np.array(stmt.key.ic)]
    acc = G1.mul(ic[0], sw)
    for j in range(len(ic) - 1):
        acc = G1.add(acc, G1.mul(ic[j + 1], sum(weights[i] * inputs_ints[i][j] for i in live) % ref.R))
    sc = None
    for i in live:
        sc = G1.add(sc, G1.mul(ref.proof_from_borsh(proofs[i].tobytes())[2], weights[i]))
    limbs = tuple(int(x) for x in np.frombuffer(ref.to_mont(sw, ref.R).to_bytes(32, 'little'), np.uint64))
    return limbs, ref.g1_raw_le(acc), ref.g1_raw_le(sc)


def explicit_weights(n, seed=5):
    """n explicit nonzero 128-bit weights (explicit weights are for tests: a service passes None)"""
    rnd = random.Random(seed)
    return [rnd.randrange(1, 1 << 128) for _ in range(n)]

