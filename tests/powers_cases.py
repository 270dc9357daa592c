"""Shared case builders of tests/test_powers_host.py and tests/test_gpu_powers.py: the secrets of a second contribution, transcripts for
given secrets MADE WITH THE ORACLE's g1_mul / g2_mul (never with the library), the expected public part, sample points of every class
-- plain byte surgery on oracle points and agg_cases' point outside the subgroup --, the tampered updates and the flags each must clear,
by reasoning.  Everything is computed once per session."""
import numpy as np

import agg_cases
import bn254_ref as ref
import ceremony_init_cases as ic
import fixtures as fx

R, Q = ref.R, ref.Q
TAU, ALPHA, BETA = ic.TAU, ic.ALPHA, ic.BETA
SEED = ic.SEED

# the secrets of the second contribution: three fixed 254-bit values
X = 0x2b0d3c5f7a91e46802c4d6f8a1b3c5d7e9f10325476980badcfe1032547698ba % R
Y = 0x1a2b3c4d5e6f708192a3b4c5d6e7f8090a1b2c3d4e5f60718293a4b5c6d7e8f9 % R
Z = 0x2f1e0d3c4b5a69788796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f1 % R
assert all(1 << 252 < v < R for v in (X, Y, Z))

g1, g2 = ic.g1, ic.g2


def mont(k):
    return fx.mont_fr(k % R)


_TRANSCRIPTS = {}


def oracle_transcript(tau, alpha, beta, m):
    """the transcript of these secrets for a domain of m, by the oracle's multiplications"""
    key = (tau % R, alpha % R, beta % R, m)
    if key not in _TRANSCRIPTS:
        from fawkes_crypto_amd import PowersOfTau
        pw = [1]
        for _ in range(2 * m - 2):
            pw.append(pw[-1] * tau % R)
        _TRANSCRIPTS[key] = PowersOfTau(np.array([g1(t) for t in pw]), np.array([g2(t) for t in pw[:m]]), np.array([g1(alpha * t) for t in pw[:m]]),
                                        np.array([g1(beta * t) for t in pw[:m]]), g2(beta))
    return _TRANSCRIPTS[key]


def before(m):
    """the transcript of TAU, ALPHA, BETA (ic.transcript's prefix)"""
    return ic.transcript().prefix(m)


def after(m):
    """what one contribution (X, Y, Z) to before(m) must give"""
    return oracle_transcript(TAU * X, ALPHA * Y, BETA * Z, m)


def public():
    from fawkes_crypto_amd import PowersPublic
    return PowersPublic(g2(X), g2(Y), g2(Z))


def same_transcript(got, want):
    for name in ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1', 'beta_g2'):
        assert getattr(got, name).shape == getattr(want, name).shape, name + ' count'
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


# ---------------------------------------------------------------------------------------------- sample points of every class
Q_LIMBS = np.frombuffer(Q.to_bytes(32, 'little'), np.uint8)


def bad_point(group, cls, salt=0):
    """one raw point of class `cls` in G1 ('g1', 64 bytes) or G2 ('g2', 128 bytes); `salt` varies the good material it is cut from"""
    mul, w = (g1, 64) if group == 'g1' else (g2, 128)
    p = mul(1000 + salt).copy()
    if cls == 'infinity':
        return np.zeros(w, np.uint8)
    if cls == 'range':              # the last coordinate's limbs are q itself (salt 0) or all ones: not below q
        p[w - 32:] = Q_LIMBS if salt % 2 == 0 else 0xff
        return p
    if cls == 'curve':              # x of one point, y of another: both in range, not on the curve
        p[w // 2:] = mul(2000 + salt)[w // 2:]
        return p
    if cls == 'subgroup':
        assert group == 'g2'
        P = agg_cases.point_outside_the_subgroup()
        if salt % 2:
            P = ref.G2.neg(P)
        return np.frombuffer(ref.g2_raw_le(P), np.uint8).copy()
    if cls == 'good':
        return p
    raise KeyError(cls)


CLASSES = dict(g1=('infinity', 'range', 'curve'), g2=('infinity', 'range', 'curve', 'subgroup'))


# ---------------------------------------------------------------------------------------------- tampered updates
OWN_FLAGS = ('shape_ok', 'points_ok', 'step_tau', 'step_alpha', 'step_beta')
TAMPERS = ic.TAMPERS + ('pub_x', 'pub_y', 'pub_z', 'other_before', 'alpha_off_curve_mid', 'tau_g2_outside_subgroup')

# The flags each tamper clears, by reasoning (not read off the code under test), for m >= 4: (own flags, flags of the embedded report).
#   ic.TAMPERS applied to `after` replace elements by other GROUP elements: points_ok stays, the embedded report loses what ic.CLEARED says
#   (the reasoning there does not depend on which secrets the honest transcript has: tau + 1 is not tau X, beta + 1 is not beta Z).  Of the
#   single points a step reads -- after.tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] -- they touch alpha_tau_g1[0] and beta_tau_g1[0] (the
#   "first" tampers of those arrays); no "mid" index is 1.
#   pub_*: [x + 1] G2 in place of [x] G2 breaks that step's equation and nothing else reads pub.
#   other_before: `after` is an honest transcript, but of (TAU + 1) X, (ALPHA + 1) Y, (BETA + 1) Z: consistent in itself, every step broken.
#   alpha_off_curve_mid: a point off the curve in the middle of after.alpha_tau_g1 is a curve failure; the array is not summed, so its
#   ratio flag is 0; alpha_tau_g1[0] is untouched.
#   tau_g2_outside_subgroup: on the curve, so it is summed and paired; it is not [tau^i] G2, so the sequence is not geometric.
CLEARED = {k: (set(), set(ic.CLEARED[k])) for k in ic.TAMPERS}
CLEARED['alpha_tau_g1_first'][0].add('step_alpha')
CLEARED['beta_tau_g1_first'][0].add('step_beta')
CLEARED.update(pub_x=({'step_tau'}, set()), pub_y=({'step_alpha'}, set()), pub_z=({'step_beta'}, set()),
               other_before=({'step_tau', 'step_alpha', 'step_beta'}, set()),
               alpha_off_curve_mid=({'points_ok'}, {'ratio_alpha'}), tau_g2_outside_subgroup=({'points_ok'}, {'ratio_tau_g2'}))
# the one bad point a tamper plants: array -> (class, index as a function of m)
BAD_POINT = dict(alpha_off_curve_mid=('alpha_tau_g1', 'curve', lambda m: m // 2), tau_g2_outside_subgroup=('tau_g2', 'subgroup', lambda m: m // 2))


def tampered(m, kind):
    """(before, after, pub) for a domain of m with one thing wrong (kind None: nothing)"""
    b, a, p = before(m), after(m), public()
    if kind is None:
        return b, a, p
    if kind in ic.TAMPERS:
        return b, ic.tamper(a, m, kind), p
    if kind.startswith('pub_'):
        n = kind[-1] + '_g2'
        return b, a, p.replace(**{n: g2(dict(x=X, y=Y, z=Z)[kind[-1]] + 1)})
    if kind == 'other_before':
        return b, oracle_transcript((TAU + 1) * X, (ALPHA + 1) * Y, (BETA + 1) * Z, m), p
    name, cls, where = BAD_POINT[kind]
    t = getattr(a, name).copy()
    assert where(m) > 1
    t[where(m)] = bad_point('g2' if name == 'tau_g2' else 'g1', cls)
    return b, a.replace(**{name: t}), p


def expect_own(kind=None):
    cleared = CLEARED[kind][0] if kind else set()
    return {n: n not in cleared for n in OWN_FLAGS}


def expect_after(kind=None):
    cleared = CLEARED[kind][1] if kind else set()
    return {n: n not in cleared for n in ic.FLAGS}


def expect_points(m, kind=None):
    """array -> (counts, first_bad)"""
    out = {n: (dict(infinity=0, range=0, curve=0, subgroup=0), None) for n in ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1', 'beta_g2')}
    if kind in BAD_POINT:
        name, cls, where = BAD_POINT[kind]
        out[name][0][cls] = 1
        out[name] = (out[name][0], where(m))
    return out


def assert_update_report(rep, m, kind):
    assert rep.flags() == expect_own(kind), kind
    assert rep.after.flags() == expect_after(kind), kind
    assert rep.accept is (kind is None)
    assert rep.after.accept is (not CLEARED[kind][1] if kind else True)
    assert {n: (r.counts(), r.first_bad) for n, r in rep.points.items()} == expect_points(m, kind)
    assert rep.changed is True
