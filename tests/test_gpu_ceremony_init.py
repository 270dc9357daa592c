"""The initial key on the device (include/fawkes_hip_ceremony_init.h through fawkes_crypto_amd/ceremony_init.py): the transforms over group
elements against their host entries and against the oracle's scalar transform mapped through its g1_mul / g2_mul, the key from a transcript
against THE ORACLE'S OWN SETUP WITH gamma = delta = 1 for every shape of tests/ceremony_init_cases.py, the chain initial key -> two
contributions against the oracle's setup with delta = x1 x2 (and the proof that key makes), the transcript check's report against the host
reference for the honest transcript and every tamper, and the refusal beside a proof that holds the lanes.  Every comparison is exact; the
transcript, the expected keys and the tampers never come from the code under test."""
import numpy as np
import pytest

import bn254_ref as ref
import c_oracle as co
import ceremony_cases as cc
import ceremony_init_cases as ic
import fawkes_crypto_amd as fk
import fixtures as fx
from fawkes_crypto_amd import ceremony, ceremony_init as CI

pytestmark = pytest.mark.gpu

R = ref.R
GROUPS = dict(g1=(co.g1_mul, CI.g1_ntt, CI.g1_ntt_dev, ic.G1, 64), g2=(co.g2_mul, CI.g2_ntt, CI.g2_ntt_dev, ic.G2, 128))


class _Dev:
    """a device buffer holding a host array, freed on exit"""

    def __init__(self, ctx, arr):
        self.ctx, self.nbytes = ctx, arr.nbytes
        self.ptr = ctx.dev_alloc(max(self.nbytes, 64))
        ctx.upload(self.ptr, np.ascontiguousarray(arr))
        ctx.sync()

    def get(self, shape):
        self.ctx.sync()
        return self.ctx.download(self.ptr, self.nbytes).reshape(shape)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.dev_free(self.ptr)


_INPUTS = {}


def _scalars(kind, n):
    """canonical Python integers; a zero gives the point at infinity"""
    if kind == 'random':
        s = [int(x) for x in np.random.default_rng(n).integers(1, 1 << 62, n)]
        return [(x * 0x9e3779b97f4a7c15f39cc0605cedc835 + i) % R for i, x in enumerate(s)]
    p = 0x1234567
    if kind == 'constant':         # out = [n]P at index 0 and infinity elsewhere: the doubling and the cancellation branch of the butterfly
        return [p] * n
    if kind == 'single':           # one point at index 1, infinity elsewhere: out[k] = omega^k P
        return [0, p] + [0] * (n - 2)
    if kind == 'holes':            # infinity at the first, a middle and the last index
        s = _scalars('random', n)
        for i in (0, n // 2, n - 1):
            s[i] = 0
        return s
    if kind == 'opposite':         # in[i] = -in[i + n / 2]
        s = _scalars('random', n)
        return s[:n // 2] + [(R - x) % R for x in s[:n // 2]]
    raise KeyError(kind)


def _inputs(group, kind, n, inverse):
    """(points, the oracle's expectation in one direction): the scalar transform of the exponents mapped through the oracle's multiplication"""
    mul, gen = GROUPS[group][0], GROUPS[group][3]

    def to_points(sc):
        return np.array([mul(gen, sc[i]) for i in range(n)])
    k = (group, kind, n)
    if k not in _INPUTS:
        s = co.limbs_arr([ref.to_mont(x, R) for x in _scalars(kind, n)])
        _INPUTS[k] = [s, to_points(s), {}]
    s, pts, want = _INPUTS[k]
    if inverse not in want:
        want[inverse] = to_points(co.fr_ntt(s, inverse=inverse))
    return pts, want[inverse]


def _transform_case(ctx, group, kind, log_n, inverse):
    ntt = GROUPS[group][1]
    pts, want = _inputs(group, kind, 1 << log_n, inverse)
    got = ntt(ctx, pts, inverse=inverse)
    assert got.tobytes() == ntt(None, pts, inverse=inverse).tobytes(), 'device against the host entry'
    assert got.tobytes() == want.tobytes(), 'device against the oracle'
    return pts, got


@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('group,log_n', [(g, k) for g in ('g1', 'g2') for k in (0, 1, 2, 5, 6, 7, 8, 11)] + [('g1', 12)])
def test_transform_equals_host_entry_and_oracle(ctx, oracle, group, log_n, inverse):
    _transform_case(ctx, group, 'random', log_n, inverse)


@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('kind', ['constant', 'single', 'holes', 'opposite'])
@pytest.mark.parametrize('group,log_n', [('g1', 6), ('g1', 7), ('g2', 6), ('g2', 7)])
def test_transform_of_structured_inputs(ctx, oracle, group, log_n, kind, inverse):
    pts, got = _transform_case(ctx, group, kind, log_n, inverse)
    n = 1 << log_n
    if kind == 'constant':
        assert got[0].any() and not got[1:].any()
        if not inverse:
            mul, gen = GROUPS[group][0], GROUPS[group][3]
            assert got[0].tobytes() == mul(gen, fx.mont_fr(n * 0x1234567)).tobytes()
    if kind == 'single':
        assert all(got[k].any() for k in range(n)) and len({got[k].tobytes() for k in range(n)}) == n
    if kind == 'opposite':
        assert not got[0::2].any()             # the even outputs are sums of in[i] + in[i + n / 2] = 0


@pytest.mark.parametrize('group', ['g1', 'g2'])
def test_transform_in_place_on_the_device(ctx, oracle, group):
    _, _, ntt_dev, _, width = GROUPS[group]
    pts, want_fwd = _inputs(group, 'holes', 64, False)
    with _Dev(ctx, pts) as d:
        ntt_dev(ctx, d.ptr, 6)
        assert d.get((64, width)).tobytes() == want_fwd.tobytes()          # the array that comes back is the only output
        ntt_dev(ctx, d.ptr, 6, inverse=True)
        assert d.get((64, width)).tobytes() == pts.tobytes()


# ---------------------------------------------------------------- the initial key
_HOST = {}


def _host_key(shape):
    if shape not in _HOST:
        _HOST[shape] = fk.initial_key_host(ic.transcript(), ic.case(shape).r1cs)
    return _HOST[shape]


@pytest.mark.parametrize('levels', [False, True])
@pytest.mark.parametrize('shape', list(ic.SHAPES))
def test_initial_key_is_the_oracles_setup(ctx, oracle, shape, levels):
    c = ic.case(shape)
    p = fk.initial_key(ctx, ic.transcript(), c.r1cs, levels=levels)
    try:
        got = dict(h=p.h, l=p.l, a=p.a, b_g1=p.b_g1, b_g2=p.b_g2)
        ic.assert_key(got, p.vk_full, p.ic, c.key)
        want = c.key
        assert p.key.counts() == dict(m=c.m, num_input=c.cs.num_input, num_aux=c.cs.num_aux, n_h=c.m - 1, n_l=c.cs.num_aux, n_a=np.array(want.a).shape[0],
                                      n_b=np.array(want.b_g1).shape[0], shard_count=1)
        if not levels:
            assert not any(p.key.precomputed().values())
        if shape == 'unused':
            assert not p.l[-1].any() and p.l[-2].any()
        if shape in ('small', 'mid'):
            h = _host_key(shape)
            for name in got:
                assert got[name].tobytes() == getattr(h, name).tobytes(), name
            assert p.ic.tobytes() == h.ic.tobytes()
    finally:
        p.key.free()


def test_chain_of_contributions_from_the_initial_key(ctx, oracle):
    c = ic.case('mid')
    x1, x2 = cc.XS['random'], cc.XS['naf255']
    p = fk.initial_key(ctx, ic.transcript(), c.r1cs)
    k1, _ = ceremony.contribute(ctx, p.key, fx.mont_fr(x1))
    k2, deltas = ceremony.contribute(ctx, k1, fx.mont_fr(x2))
    try:
        want = c.expected(x1 * x2 % R)
        got = {n: k2.download(n) for n in ('h', 'l', 'a', 'b_g1', 'b_g2')}
        vk = dict(p.vk_full, **deltas)
        ic.assert_key(got, vk, p.ic, want)
        assert ceremony.check(ctx, p.key, k1, cc.SEED).accept and ceremony.check(ctx, k1, k2, cc.SEED).accept
        # the final key proves what the oracle proves with its key for delta = x1 x2, and the proof verifies with gamma_g2 = the generator
        z = fx.witness_mont(c.z_in, c.z_aux)
        a, b, c_, aa, bi, ba = oracle.synthesize(c.csr, z)
        r, s = fx.mont_fr(0xace), fx.mont_fr(0xbee)
        proof = ctx.prove_raw(k2, a, b, c_, z, aa, bi, ba, r, s).tobytes()
        assert proof == oracle.prove(want, a, b, c_, z, aa, bi, ba, r, s).tobytes()
        assert vk['gamma_g2'].tobytes() == ic.G2.tobytes()
        assert fk.verify(fk.vk_to_borsh(vk), z[1:c.cs.num_input], proof) is True
        assert fk.verify(fk.vk_to_borsh(p.vk_full), z[1:c.cs.num_input], proof) is False          # not under the initial key's delta
    finally:
        k2.free(); k1.free(); p.key.free()


def test_image_to_image(ctx, oracle):
    """a `Parameters` image of the circuit under SOME key (helpers.TOXIC's, with its own gamma and delta) -> the image of the initial key"""
    from fawkes_crypto_amd import params_io as pio
    from helpers import TOXIC
    c = ic.case('small')
    k = co.setup(c.csr, **TOXIC)
    arrays = dict(alpha_g1=k.alpha_g1, beta_g1=k.beta_g1, beta_g2=k.beta_g2, gamma_g2=k.gamma_g2, delta_g1=k.delta_g1, delta_g2=k.delta_g2,
                  ic=np.array(k.ic), h=np.array(k.h), l=np.array(k.l), a=np.array(k.a), b_g1=np.array(k.b_g1), b_g2=np.array(k.b_g2))
    image = pio.store_parameters(arrays, c.r1cs, const_tracker_bits=[True, False, True])
    new_image = fk.initial_image(ctx, ic.transcript(), image)
    assert isinstance(new_image, bytes) and len(new_image) == len(image)
    key, dr, hdr = pio.load_parameters(ctx, new_image, checked=True, warm=False)
    try:
        got = {n: key.download(n) for n in ('h', 'l', 'a', 'b_g1', 'b_g2')}
        ic.assert_key(got, dict(key.vk(), gamma_g2=hdr['gamma_g2']), hdr['ic'], c.key)
        assert hdr['const_tracker'] == [True, False, True]
        h0, h1 = pio.read_parameters(image), pio.read_parameters(new_image)
        assert bytes(h0['gates_blob']) == bytes(h1['gates_blob'])
    finally:
        dr.free(); key.free()


# ---------------------------------------------------------------- the transcript check
def _same_report(dev, host):
    assert dev.flags() == host.flags() and dev.accept == host.accept
    assert dev.sums() == host.sums() and dev.seed == host.seed


@pytest.mark.parametrize('kind', (None,) + ic.TAMPERS)
@pytest.mark.parametrize('m', [64, 1 << 11])
def test_check_report_equals_the_host_reference(ctx, oracle, m, kind):
    pw = ic.transcript() if kind is None else ic.tamper(ic.transcript(), m, kind)
    rep = fk.check_powers(ctx, pw, m, ic.SEED)
    assert rep.flags() == ic.expect_flags(kind) and rep.accept is (kind is None)
    _same_report(rep, fk.check_powers_host(pw, m, ic.SEED))


def test_check_draws_its_own_seed(ctx, oracle):
    pw = ic.transcript()
    r1, r2 = fk.check_powers(ctx, pw, 64), fk.check_powers(ctx, pw, 64)
    assert r1.accept and r2.accept and r1.seed != r2.seed and r1.s_tau_g1 != r2.s_tau_g1
    _same_report(fk.check_powers(ctx, pw, 64, r1.seed), r1)


# ---------------------------------------------------------------- guards
def test_guards(ctx, oracle):
    c = ic.case('small')
    pw = ic.transcript()

    def refused(fn, code=1):
        with pytest.raises(fk.FkError) as e:
            fn()
        assert e.value.code == code

    refused(lambda: fk.initial_key(ctx, pw.prefix(32), c.r1cs))                     # too short for m = 64
    refused(lambda: fk.check_powers(ctx, pw.prefix(32), 64, ic.SEED))
    # a proof that holds the lanes between two calls
    params = fk.initial_key(ctx, pw, c.r1cs)
    dk = params.key
    dr = ctx.load_r1cs(c.r1cs)
    z = fx.witness_mont(c.z_in, c.z_aux)
    a, b, c_, aa, bi, ba = oracle.synthesize(c.csr, z)
    r, s = fx.mont_fr(0xace), fx.mont_fr(0xbee)
    old = ctx.prove_raw(dk, a, b, c_, z, aa, bi, ba, r, s).tobytes()
    assert old == oracle.prove(c.key, a, b, c_, z, aa, bi, ba, r, s).tobytes()
    with _Dev(ctx, z) as d_z, _Dev(ctx, np.zeros((c.m, 4), np.uint64)) as d_h:
        ctx.prove_msms_z_begin_dev(dk, d_z.ptr, *dr.density_ptrs())
        try:
            refused(lambda: fk.initial_key(ctx, pw, c.r1cs))
            refused(lambda: fk.check_powers(ctx, pw, 64, ic.SEED))
        finally:
            ctx.prove_msms_finish_dev(dk, d_h.ptr)
    # the context is still usable: the old bytes, and both entries again
    assert ctx.prove_raw(dk, a, b, c_, z, aa, bi, ba, r, s).tobytes() == old
    assert fk.check_powers(ctx, pw, 64, ic.SEED).accept
    again = fk.initial_key(ctx, pw, c.r1cs)
    assert again.h.tobytes() == params.h.tobytes()
    again.key.free(); dr.free(); dk.free()
