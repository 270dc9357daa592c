"""Shared case builders of tests/test_ceremony_host.py and tests/test_gpu_ceremony.py: keys from the oracle's setup over ref.random_r1cs
(as tests/test_gpu_setup.py builds them), the scalars, the expected contributed key -- THE ORACLE'S OWN SETUP WITH delta * x mod r, never
the code under test --, the tampered keys of a check with the flags each must clear, and the Python restatements (weights through
oracle/fawkes_circuit.py's chacha20_block, sums over ref.G1, verdicts through ref's pairing).  Everything is computed once per session."""
import numpy as np

import bn254_ref as ref
import c_oracle as co
import fawkes_circuit as fc
import fixtures as fx
from helpers import params_from_oracle_key, r1cs_product, TOXIC

R = ref.R
SEED = bytes(range(1, 33))
OTHER_SEED = bytes(range(101, 133))

# name -> (seed, gates, inputs, aux); 'big' gives m = 2^14 and many workgroups
SHAPES = dict(tiny=(1, 3, 1, 5), small=(2, 60, 3, 70), mid=(3, 900, 2, 1000), big=(4, 8000, 3, 8100))

# x of a contribution.  r - 1 and r - 5 have a non-adjacent form of 255 digits (naf_len below says so); 'random' is a fixed 254-bit value
XS = dict(one=1, two=2, r_minus_1=R - 1, random=0x2b0d3c5f7a91e46802c4d6f8a1b3c5d7e9f10325476980badcfe1032547698ba % R, naf255=R - 5)

FLAGS = ('shape_equal', 'fixed_equal', 'delta_nonzero', 'delta_pair', 'ratio_h', 'ratio_l')


def naf_len(k):
    """digits of the non-adjacent form of k"""
    n = 0
    while k:
        if k & 1:
            k -= 2 - (k & 3)
        k >>= 1
        n += 1
    return n


assert naf_len(XS['naf255']) == 255 and naf_len(XS['r_minus_1']) == 255 and XS['random'].bit_length() == 254


class Case:
    """One circuit and its oracle key.  unused_aux: one more aux variable that occurs in no constraint, so that l ends in the point
    at infinity."""

    def __init__(self, shape, unused_aux=False):
        seed, gates, nin, naux = SHAPES[shape]
        cs, self.z_in, self.z_aux = ref.random_r1cs(seed, gates, nin, naux)
        if unused_aux:
            cs = ref.R1CS(cs.num_input, cs.num_aux + 1, cs.rows)
            self.z_aux = list(self.z_aux) + [0]
        self.cs, self.csr = cs, fx.r1cs_to_csr(cs)
        self.r1cs = r1cs_product(self.csr)
        self.key = co.setup(self.csr, **TOXIC)
        self.params = params_from_oracle_key(self.key, self.r1cs)
        self._expected = {}

    def expected(self, x):
        """the oracle's key for delta * x: what a contribution with x must give, byte for byte"""
        if x not in self._expected:
            tw = dict(TOXIC, delta=TOXIC['delta'] * x % R)
            self._expected[x] = co.setup(self.csr, **tw)
        return self._expected[x]

    def expected_params(self, x):
        return params_from_oracle_key(self.expected(x), self.r1cs)


_CASES = {}


def case(shape, unused_aux=False):
    k = (shape, unused_aux)
    if k not in _CASES:
        _CASES[k] = Case(shape, unused_aux)
    return _CASES[k]


def clone(params, **over):
    """a copy of an api.Parameters with some arrays / vk points replaced"""
    import fawkes_crypto_amd as fk
    arrays = dict(m=params.m, num_input=params.num_input, num_aux=params.num_aux, h=params.h.copy(), l=params.l.copy(), a=params.a.copy(),
                  b_g1=params.b_g1.copy(), b_g2=params.b_g2.copy())
    arrays.update({n: v.copy() for n, v in params.vk.items()})
    arrays.update(over)
    return fk.Parameters(arrays, params.r1cs)


def assert_contributed(got, case_, x, a=None, b_g1=None, b_g2=None):
    """got: dict(h, l, delta_g1, delta_g2[, a, b_g1, b_g2, alpha_g1, beta_g1, beta_g2]) of raw bytes against the oracle's key for delta x"""
    want = case_.expected(x)
    for name in ('h', 'l'):
        assert np.asarray(got[name]).tobytes() == np.array(getattr(want, name)).tobytes(), name
    for name in ('delta_g1', 'delta_g2'):
        assert np.asarray(got[name]).tobytes() == getattr(want, name).tobytes(), name
    for name in ('a', 'b_g1', 'b_g2'):
        if name in got:
            assert np.asarray(got[name]).tobytes() == np.array(getattr(case_.key, name)).tobytes() == np.array(getattr(want, name)).tobytes(), name
    for name in ('alpha_g1', 'beta_g1', 'beta_g2'):
        if name in got:
            assert np.asarray(got[name]).tobytes() == getattr(case_.key, name).tobytes(), name


# ---------------------------------------------------------------------------------------------- tampered keys
TAMPERS = ('h_first', 'h_mid', 'h_last', 'l_double', 'l_swap', 'delta_g2_other', 'a_changed', 'counts', 'delta_inf')

# the flags each tamper clears, by reasoning (not read off the code under test):
#   a doubled h' (l') element breaks the h (l) ratio and nothing else; so does a swap of two different l' elements
#   delta_g2' = [x + 1] delta_g2 beside delta_g1' = [x] delta_g1: the two deltas no longer pair, and h' = [1/x] h is not [1/(x+1)] h
#   a changed `a` element: only the fixed part differs
#   unequal counts: the arrays cannot be paired up -- shape_equal, and with it fixed_equal and both ratios, are not established
#   both deltas at infinity: e(G1, 0) = e(0, G2) = 1 still "pair"; e(S', 0) = 1 is not e(S, delta_g2) for S != 0
CLEARED = dict(h_first={'ratio_h'}, h_mid={'ratio_h'}, h_last={'ratio_h'}, l_double={'ratio_l'}, l_swap={'ratio_l'},
               delta_g2_other={'delta_pair', 'ratio_h', 'ratio_l'}, a_changed={'fixed_equal'},
               counts={'shape_equal', 'fixed_equal', 'ratio_h', 'ratio_l'}, delta_inf={'delta_nonzero', 'ratio_h', 'ratio_l'})


def _dbl(p):
    return co.g1_add(p, p)


def tamper(case_, after, kind, x):
    """`after` (an honest contribution with x to case_.params) with one thing wrong"""
    h, l = after.h.copy(), after.l.copy()
    finite = [i for i in range(l.shape[0]) if l[i].any()]
    if kind in ('h_first', 'h_mid', 'h_last'):
        i = dict(h_first=0, h_mid=h.shape[0] // 2, h_last=h.shape[0] - 1)[kind]
        assert h[i].any()
        h[i] = _dbl(h[i])
        return clone(after, h=h)
    if kind == 'l_double':
        i = finite[len(finite) // 2]
        l[i] = _dbl(l[i])
        return clone(after, l=l)
    if kind == 'l_swap':
        i = finite[0]
        j = next(j for j in finite[1:] if l[j].tobytes() != l[i].tobytes())
        l[[i, j]] = l[[j, i]]
        return clone(after, l=l)
    if kind == 'delta_g2_other':
        return clone(after, delta_g2=co.g2_mul(case_.params.vk['delta_g2'], fx.mont_fr(x + 1)))
    if kind == 'a_changed':
        a = after.a.copy()
        a[a.shape[0] // 2] = _dbl(a[a.shape[0] // 2])
        return clone(after, a=a)
    if kind == 'counts':
        return clone(after, a=after.a[:-1].copy())
    if kind == 'delta_inf':
        return clone(after, delta_g1=np.zeros(64, np.uint8), delta_g2=np.zeros(128, np.uint8))
    raise KeyError(kind)


def expect_flags(kind=None):
    cleared = CLEARED[kind] if kind else set()
    return {n: n not in cleared for n in FLAGS}


# ---------------------------------------------------------------------------------------------- Python restatements
def weights_py(seed, n):
    """the n weights as Python integers: words 4 (i mod 4) .. + 3 of block i / 4 of chacha20_block(key = seed, counter, stream 0)"""
    key = [int.from_bytes(seed[4 * i:4 * i + 4], 'little') for i in range(8)]
    out, blk = [], None
    for i in range(n):
        if i % 4 == 0:
            blk = fc.chacha20_block(key, i // 4, 0)
        w = sum(blk[4 * (i % 4) + j] << (32 * j) for j in range(4))
        out.append(w or 1)
    return out


def weights_mont_py(seed, n):
    ws = weights_py(seed, n)
    return co.limbs_arr([ref.to_mont(w, R) for w in ws]) if n else np.zeros((0, 4), np.uint64)


def sum_py(points, ws):
    """sum ws[i] * points[i] over ref.G1 as 64 raw bytes"""
    acc = ref.G1.jac_inf()
    for row, w in zip(points, ws):
        p = ref.g1_from_raw_le(row.tobytes())
        if p is not None:
            acc = ref.G1.jac_add(acc, ref.G1.jac_mul(ref.G1.to_jac(p), w))
    return ref.g1_raw_le(ref.G1.to_affine(acc))


def pairing_eq_py(p1, q1, p2, q2):
    """e(p1, q1) == e(p2, q2) over raw bytes, by ref's pairing"""
    g1, g2 = lambda b: ref.g1_from_raw_le(bytes(b)), lambda b: ref.g2_from_raw_le(bytes(b))
    f = ref.f12_mul(ref.miller_loop(g2(q1), g1(p1)), ref.miller_loop(g2(q2), ref.G1.neg(g1(p2))))
    return ref.final_exp(f) == ref.f12_one()


def verdicts_py(before, after, rep):
    """delta_pair, ratio_h, ratio_l by the Python pairing, over the report's own sums (the sums are checked separately)"""
    gen1, gen2 = ref.g1_raw_le(ref.G1_GEN), ref.g2_raw_le(ref.G2_GEN)
    return dict(delta_pair=pairing_eq_py(after.vk['delta_g1'], gen2, gen1, after.vk['delta_g2']),
                ratio_h=pairing_eq_py(rep.s_h_after, after.vk['delta_g2'], rep.s_h, before.vk['delta_g2']),
                ratio_l=pairing_eq_py(rep.s_l_after, after.vk['delta_g2'], rep.s_l, before.vk['delta_g2']))
