"""The key ceremony's host references (include/fawkes_hip_ceremony.h through fawkes_crypto_amd/ceremony.py; no GPU): the weights against
a Python derivation, a contribution against THE ORACLE'S OWN SETUP WITH delta * x, the check's sums against Python integers over ref.G1
and its verdicts against the Python pairing, every tamper with exactly its flags cleared, the attack the secret weights exist for, and
the argument errors.  Every comparison is exact."""
import numpy as np
import pytest

import bn254_ref as ref
import ceremony_cases as cc
import fixtures as fx


def _cer():
    from fawkes_crypto_amd import ceremony
    return ceremony


def _x(name):
    return fx.mont_fr(cc.XS[name])


_AFTER = {}


def _after(shape, unused, xname):
    """one honest host contribution per (case, x) per session"""
    k = (shape, unused, xname)
    if k not in _AFTER:
        _AFTER[k] = _cer().contribute_host(cc.case(shape, unused).params, _x(xname))
    return _AFTER[k]


@pytest.mark.parametrize('n', [0, 1, 4, 5, 9])
def test_weights_are_the_chacha20_words(oracle, n):
    got = _cer().weights(cc.SEED, n)
    assert got.shape == (n, 4) and got.tobytes() == cc.weights_mont_py(cc.SEED, n).tobytes()
    if n:
        assert got.tobytes() != _cer().weights(cc.OTHER_SEED, n).tobytes()
        assert all(0 < w < 1 << 128 for w in cc.weights_py(cc.SEED, n))


def test_scale_host_against_the_oracle(oracle):
    c = cc.case('tiny', True)
    pts = np.concatenate([np.zeros((1, 64), np.uint8), np.array(c.key.h), np.array(c.key.l)])
    for xname in ('one', 'two', 'r_minus_1', 'random', 'naf255'):
        got = _cer().scale_g1(None, pts, _x(xname))
        for i in range(len(pts)):
            assert got[i].tobytes() == oracle.g1_mul(pts[i], _x(xname)).tobytes(), (xname, i)
    assert not _cer().scale_g1(None, pts, fx.mont_fr(0)).any()
    assert _cer().scale_g1(None, np.zeros((0, 64), np.uint8), _x('two')).shape == (0, 64)


@pytest.mark.parametrize('xname', ['one', 'two', 'r_minus_1', 'random'])
@pytest.mark.parametrize('shape,unused', [('tiny', False), ('tiny', True), ('small', False)])
def test_contribution_is_the_oracles_setup_with_delta_x(oracle, shape, unused, xname):
    c = cc.case(shape, unused)
    if unused:
        assert not np.array(c.key.l)[-1].any(), 'the unused variable must give the point at infinity in l'
    after = _after(shape, unused, xname)
    cc.assert_contributed(dict(h=after.h, l=after.l, a=after.a, b_g1=after.b_g1, b_g2=after.b_g2, **after.vk), c, cc.XS[xname])
    if unused:
        assert not after.l[-1].any()
    # the input is untouched
    assert c.params.h.tobytes() == np.array(c.key.h).tobytes() and c.params.vk['delta_g1'].tobytes() == c.key.delta_g1.tobytes()


@pytest.mark.parametrize('shape,unused,xname', [('tiny', False, 'random'), ('tiny', True, 'two'), ('tiny', False, 'one'), ('small', False, 'r_minus_1')])
def test_check_accepts_a_contribution(oracle, shape, unused, xname):
    c = cc.case(shape, unused)
    after = _after(shape, unused, xname)
    rep = _cer().check_host(c.params, after, cc.SEED)
    assert rep.flags() == cc.expect_flags() and rep.accept is True
    assert rep.delta_changed is (xname != 'one') and rep.seed == cc.SEED
    if shape == 'tiny':
        ws = cc.weights_py(cc.SEED, max(c.params.h.shape[0], c.params.l.shape[0]))
        assert rep.s_h == cc.sum_py(c.params.h, ws) and rep.s_h_after == cc.sum_py(after.h, ws)
        assert rep.s_l == cc.sum_py(c.params.l, ws) and rep.s_l_after == cc.sum_py(after.l, ws)
        assert cc.verdicts_py(c.params, after, rep) == dict(delta_pair=True, ratio_h=True, ratio_l=True)
    # the weights depend on the seed, the verdict does not
    rep2 = _cer().check_host(c.params, after, cc.OTHER_SEED)
    assert rep2.accept is True and rep2.s_h != rep.s_h


def test_check_accepts_a_chain_of_two(oracle):
    c = cc.case('tiny')
    first = _after('tiny', False, 'random')
    second = _cer().contribute_host(first, _x('two'))
    cc.assert_contributed(dict(h=second.h, l=second.l, **second.vk), c, cc.XS['random'] * 2 % cc.R)
    assert _cer().check_host(first, second, cc.SEED).accept is True
    # the check composes: the second key is also the first one's ancestor contributed to once, with x = random * 2
    assert _cer().check_host(c.params, second, cc.SEED).accept is True
    # backwards it is a contribution too, with 1 / 2: the check says THAT a key descends from another, not in which order they were made
    assert _cer().check_host(second, first, cc.SEED).accept is True
    assert _cer().check_host(second, second, cc.SEED).delta_changed is False


@pytest.mark.parametrize('kind', cc.TAMPERS)
def test_check_rejects_with_exactly_the_expected_flags(oracle, kind):
    c = cc.case('small')
    after = _after('small', False, 'random')
    bad = cc.tamper(c, after, kind, cc.XS['random'])
    rep = _cer().check_host(c.params, bad, cc.SEED)
    assert rep.flags() == cc.expect_flags(kind), kind
    assert rep.accept is False


@pytest.mark.parametrize('kind', ['h_first', 'delta_g2_other'])
def test_verdicts_are_the_python_pairings(oracle, kind):
    c = cc.case('tiny')
    after = _after('tiny', False, 'random')
    bad = cc.tamper(c, after, kind, cc.XS['random'])
    rep = _cer().check_host(c.params, bad, cc.SEED)
    want = cc.verdicts_py(c.params, bad, rep)
    assert {n: getattr(rep, n) for n in want} == want
    assert want == {n: v for n, v in cc.expect_flags(kind).items() if n in want}


def test_known_weights_let_a_tamper_through(oracle):
    """THE ATTACK THE SECRET WEIGHTS EXIST FOR: h'[0] += D, h'[1] -= (rho_0 / rho_1) D cancels in sum rho_i h'[i] for whoever knows rho"""
    c = cc.case('tiny')
    after = _after('tiny', False, 'random')
    rho = cc.weights_py(cc.SEED, 2)
    coeff = rho[0] * pow(rho[1], -1, cc.R) % cc.R
    gen = np.frombuffer(ref.g1_raw_le(ref.G1_GEN), np.uint8)
    h = after.h.copy()
    h[0] = oracle.g1_add(h[0], gen)
    h[1] = oracle.g1_add(h[1], oracle.g1_mul(gen, fx.mont_fr(cc.R - coeff)))
    bad = cc.clone(after, h=h)
    assert bad.h.tobytes() != after.h.tobytes()
    assert _cer().check_host(c.params, bad, cc.SEED).accept is True
    rep = _cer().check_host(c.params, bad, cc.OTHER_SEED)
    assert rep.flags() == cc.expect_flags('h_first') and rep.accept is False


def test_argument_errors(oracle):
    from fawkes_crypto_amd import FkError
    cer = _cer()
    c = cc.case('tiny')
    with pytest.raises(FkError) as e:
        cer.contribute_host(c.params, fx.mont_fr(0))
    assert e.value.code == 1
    not_below_r = np.frombuffer(int(cc.R).to_bytes(32, 'little'), np.uint64).copy()
    with pytest.raises(FkError) as e:
        cer.contribute_host(c.params, not_below_r)
    assert e.value.code == 7
    with pytest.raises(FkError) as e:
        cer.scale_g1(None, np.array(c.key.h), not_below_r)
    assert e.value.code == 7

    class Sharded:
        def __init__(self, p):
            self.p = p

        def desc(self):
            return self.p.desc(0, 2)
    after = _after('tiny', False, 'two')
    for before, aft in ((Sharded(c.params), after), (c.params, Sharded(after))):
        with pytest.raises(FkError) as e:
            cer.check_host(before, aft, cc.SEED)
        assert e.value.code == 1
    with pytest.raises(ValueError):
        cer.check_host(c.params, after, b'short')
