"""Shared case builders of tests/test_ceremony_init_host.py and tests/test_gpu_ceremony_init.py: circuits from ref.random_r1cs (as
tests/ceremony_cases.py builds them), ONE powers-of-tau transcript for helpers.TOXIC's tau, alpha, beta -- made with the oracle's g1_mul /
g2_mul from the generators, never with the library, long enough for m = 2^11 and used by its prefixes everywhere --, the expected key
-- THE ORACLE'S OWN SETUP WITH gamma = delta = 1 --, the tampered transcripts of a check with the flags each must clear, and the Python
restatements of the check's sums and verdicts.  Everything is computed once per session."""
import numpy as np

import bn254_ref as ref
import c_oracle as co
import ceremony_cases as cc
import fixtures as fx
from helpers import r1cs_product, TOXIC

R = ref.R
SEED, OTHER_SEED = cc.SEED, cc.OTHER_SEED
TAU, ALPHA, BETA = TOXIC['tau'] % R, TOXIC['alpha'] % R, TOXIC['beta'] % R
M_MAX = 1 << 11

G1 = np.frombuffer(ref.g1_raw_le(ref.G1_GEN), np.uint8).copy()
G2 = np.frombuffer(ref.g2_raw_le(ref.G2_GEN), np.uint8).copy()

# name -> (seed, gates, inputs, aux)
SHAPES = dict(one=(11, 1, 1, 2), tiny=(12, 3, 1, 5), small=(13, 60, 3, 70), wave=(14, 125, 3, 140), mid=(15, 900, 2, 1000), big=(16, 1500, 3, 1600),
              heavy=(17, 900, 2, 1000), unused=(13, 60, 3, 70))
DOMAIN = dict(one=2, tiny=4, small=64, wave=128, mid=1024, big=2048, heavy=1024, unused=64)

# the coefficients of the heavy column, in turn: ONE, r - 1 and two full-width values
HEAVY_COEFFS = (1, R - 1, 0x2b0d3c5f7a91e46802c4d6f8a1b3c5d7e9f10325476980badcfe1032547698ba % R, 0x1a2b3c4d5e6f708192a3b4c5d6e7f8090a1b2c3d4e5f60718293a4b5c6d7e8f9 % R)
SEGMENT = 16          # csrc/ceremony_init.hip: CI_SEG -- the heavy column (900 terms) is longer and no multiple of it


def g1(k):
    return co.g1_mul(G1, fx.mont_fr(k % R))


def g2(k):
    return co.g2_mul(G2, fx.mont_fr(k % R))


_TRANSCRIPT = []


def transcript():
    """the transcript for M_MAX: 2 M_MAX - 1 powers in tau_g1, M_MAX in the others"""
    if not _TRANSCRIPT:
        from fawkes_crypto_amd import PowersOfTau
        pw = [1]
        for _ in range(2 * M_MAX - 2):
            pw.append(pw[-1] * TAU % R)
        _TRANSCRIPT.append(PowersOfTau(np.array([g1(t) for t in pw]), np.array([g2(t) for t in pw[:M_MAX]]), np.array([g1(ALPHA * t) for t in pw[:M_MAX]]),
                                       np.array([g1(BETA * t) for t in pw[:M_MAX]]), g2(BETA)))
    return _TRANSCRIPT[0]


class Case:
    """One circuit and the oracle's key for it with gamma = delta = 1."""

    def __init__(self, shape):
        seed, gates, nin, naux = SHAPES[shape]
        cs, self.z_in, self.z_aux = ref.random_r1cs(seed, gates, nin, naux)
        if shape == 'heavy':
            # one more aux variable in A of every gate, coefficients in turn; ONE in C of every gate
            v, rows = ('a', cs.num_aux), []
            for g, (A, B, Cm) in enumerate(cs.rows):
                Cm = list(Cm) + ([] if any(var == ('i', 0) for _, var in Cm) else [(1, ('i', 0))])
                rows.append((list(A) + [(HEAVY_COEFFS[g % 4], v)], B, Cm))
            cs = ref.R1CS(cs.num_input, cs.num_aux + 1, rows)
            self.z_aux = list(self.z_aux) + [0]
            assert gates > SEGMENT and gates % SEGMENT
        if shape == 'unused':
            # one aux variable in B only (of the first gate), one in no constraint at all
            (A, B, Cm), v = cs.rows[0], ('a', cs.num_aux)
            cs = ref.R1CS(cs.num_input, cs.num_aux + 2, [(A, list(B) + [(HEAVY_COEFFS[2], v)], Cm)] + list(cs.rows[1:]))
            self.z_aux = list(self.z_aux) + [0, 0]
        self.shape, self.cs, self.csr = shape, cs, fx.r1cs_to_csr(cs)
        self.r1cs = r1cs_product(self.csr)
        self.m = DOMAIN[shape]
        self.key = co.setup(self.csr, TAU, ALPHA, BETA, 1, 1)
        assert self.key.m == self.m
        self._expected = {}

    def expected(self, x):
        """the oracle's key for delta = x (gamma = 1): what a chain of contributions with product x must give, byte for byte"""
        if x not in self._expected:
            self._expected[x] = co.setup(self.csr, TAU, ALPHA, BETA, 1, x % R)
        return self._expected[x]


_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def assert_key(got, vk, ic, key):
    """got: dict of the five arrays; vk: dict of the six points; ic -- against the oracle key, byte for byte"""
    for name in ('h', 'l', 'a', 'b_g1', 'b_g2'):
        assert np.asarray(got[name]).shape[0] == np.array(getattr(key, name)).shape[0], name + ' count'
        assert np.asarray(got[name]).tobytes() == np.array(getattr(key, name)).tobytes(), name
    for name in ('alpha_g1', 'beta_g1', 'beta_g2', 'gamma_g2', 'delta_g1', 'delta_g2'):
        assert np.asarray(vk[name]).tobytes() == getattr(key, name).tobytes(), name
    assert np.asarray(ic).tobytes() == np.array(key.ic).tobytes(), 'ic'


# ---------------------------------------------------------------------------------------------- tampered transcripts
FLAGS = ('gen_ok', 'tau_pair', 'ratio_tau_g1', 'ratio_tau_g2', 'ratio_alpha', 'ratio_beta', 'beta_pair')
ARRAYS = ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1')
TAMPERS = tuple('%s_%s' % (a, w) for a in ARRAYS for w in ('first', 'mid', 'last')) + ('tau_g1_swap', 'beta_g2_other', 'tau_g2_1_other', 'tau_g1_0_other')

# The flags each tamper clears, by reasoning (not read off the code under test), for m >= 4 so that no "mid" index is 1:
#   an element that breaks the geometric sequence of its array clears that array's ratio and nothing else, unless it is one of the
#   single points another predicate reads: tau_g1[0] and tau_g2[0] (gen_ok), beta_tau_g1[0] (beta_pair; nothing reads alpha_tau_g1[0]).
#   tau_g1[1] and tau_g2[1] are touched only by tau_g2_1_other: tau_g2[1] = [tau + 1] G2 no longer pairs with tau_g1[1], is not the ratio
#   of any G1 array, and tau_g2 itself stops being geometric.  beta_g2 = [beta + 1] G2 only fails to pair with beta_tau_g1[0].
_RATIO = dict(tau_g1='ratio_tau_g1', tau_g2='ratio_tau_g2', alpha_tau_g1='ratio_alpha', beta_tau_g1='ratio_beta')
CLEARED = {}
for _a in ARRAYS:
    for _w in ('first', 'mid', 'last'):
        CLEARED['%s_%s' % (_a, _w)] = {_RATIO[_a]}
CLEARED['tau_g1_first'] |= {'gen_ok'}
CLEARED['tau_g2_first'] |= {'gen_ok'}
CLEARED['beta_tau_g1_first'] |= {'beta_pair'}
CLEARED.update(tau_g1_swap={'ratio_tau_g1'}, beta_g2_other={'beta_pair'}, tau_g1_0_other={'gen_ok', 'ratio_tau_g1'},
               tau_g2_1_other={'tau_pair', 'ratio_tau_g1', 'ratio_tau_g2', 'ratio_alpha', 'ratio_beta'})


def checked_len(name, m):
    return 2 * m - 1 if name == 'tau_g1' else m


def tamper(powers, m, kind):
    """the m-prefix of `powers` with one thing wrong"""
    p = powers.prefix(m)
    if kind == 'beta_g2_other':
        return p.replace(beta_g2=g2(BETA + 1))
    if kind == 'tau_g2_1_other':
        t = p.tau_g2.copy()
        t[1] = g2(TAU + 1)
        return p.replace(tau_g2=t)
    if kind == 'tau_g1_0_other':
        t = p.tau_g1.copy()
        t[0] = g1(3)
        return p.replace(tau_g1=t)
    if kind == 'tau_g1_swap':
        t = p.tau_g1.copy()
        assert t[5].tobytes() != t[6].tobytes()
        t[[5, 6]] = t[[6, 5]]
        return p.replace(tau_g1=t)
    name, where = kind.rsplit('_', 1)
    n = checked_len(name, m)
    i = dict(first=0, mid=n // 2, last=n - 1)[where]
    assert i != 1
    t = getattr(p, name).copy()
    t[i] = co.g1_add(t[i], t[i]) if name != 'tau_g2' else co.g2_add(t[i], t[i])
    return p.replace(**{name: t})


def expect_flags(kind=None):
    cleared = CLEARED[kind] if kind else set()
    return {n: n not in cleared for n in FLAGS}


# ---------------------------------------------------------------------------------------------- Python restatements
def sums_py(powers, m, seed):
    """the eight sums over Python integers: S = sum_{i < n - 1} rho_i T[i], S' = sum_{i < n - 1} rho_i T[i + 1]"""
    ws = cc.weights_py(seed, 2 * m - 2)
    out = {}
    for name, key in (('tau_g1', 's_tau_g1'), ('alpha_tau_g1', 's_alpha'), ('beta_tau_g1', 's_beta')):
        t = getattr(powers, name)
        n = checked_len(name, m)
        out[key], out[key + '_next'] = cc.sum_py(t[:n - 1], ws), cc.sum_py(t[1:n], ws)
    for key, rows in (('s_tau_g2', powers.tau_g2[:m - 1]), ('s_tau_g2_next', powers.tau_g2[1:m])):
        acc = ref.G2.jac_inf()
        for row, w in zip(rows, ws):
            p = ref.g2_from_raw_le(row.tobytes())
            if p is not None:
                acc = ref.G2.jac_add(acc, ref.G2.jac_mul(ref.G2.to_jac(p), w))
        out[key] = ref.g2_raw_le(ref.G2.to_affine(acc))
    return out


def verdicts_py(powers, rep):
    """the six pairing predicates by ref's pairing, over the report's own sums (the sums are checked separately)"""
    def eq(p1, q1, p2, q2):
        return cc.pairing_eq_py(p1, q1, p2, q2)
    t2 = powers.tau_g2[1]
    return dict(tau_pair=eq(powers.tau_g1[1], G2, G1, t2), ratio_tau_g1=eq(rep.s_tau_g1_next, G2, rep.s_tau_g1, t2), ratio_alpha=eq(rep.s_alpha_next, G2, rep.s_alpha, t2),
                ratio_beta=eq(rep.s_beta_next, G2, rep.s_beta, t2), ratio_tau_g2=eq(powers.tau_g1[1], rep.s_tau_g2, G1, rep.s_tau_g2_next),
                beta_pair=eq(powers.beta_tau_g1[0], G2, G1, powers.beta_g2))
