"""The key ceremony on the device (include/fawkes_hip_ceremony.h through fawkes_crypto_amd/ceremony.py): the scale kernel and the weights
kernel against their host entries byte for byte, a contribution against THE ORACLE'S OWN SETUP WITH delta * x (and the proofs the new
key makes), the check's report against the host reference for the honest key and every tamper, image to image, and the guards.  Every
comparison is exact; the expected keys and the tampers come from tests/ceremony_cases.py, never from the code under test."""
import numpy as np
import pytest

import bn254_ref as ref
import ceremony_cases as cc
import fixtures as fx
from helpers import g1_bases

pytestmark = pytest.mark.gpu


def _cer():
    from fawkes_crypto_amd import ceremony
    return ceremony


def _x(name):
    return fx.mont_fr(cc.XS[name])


class _Dev:
    """a device buffer holding a host array, freed on exit"""

    def __init__(self, ctx, arr=None, nbytes=None):
        self.ctx = ctx
        self.nbytes = arr.nbytes if arr is not None else nbytes
        self.ptr = ctx.dev_alloc(max(self.nbytes, 64))
        if arr is not None and arr.nbytes:
            ctx.upload(self.ptr, np.ascontiguousarray(arr))
            ctx.sync()                       # the copy is asynchronous and `arr` may be a temporary

    def get(self, shape):
        self.ctx.sync()
        return self.ctx.download(self.ptr, self.nbytes).reshape(shape) if self.nbytes else np.zeros(shape, np.uint8)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.dev_free(self.ptr)


_POINTS, _SCALED = {}, {}


def _points(n):
    """n points with the point at infinity in the first, a middle and the last lane (n >= 3), or in the only lane but one (n == 2)"""
    if n not in _POINTS:
        p = g1_bases(n, seed=n).copy() if n else np.zeros((0, 64), np.uint8)
        if n >= 3:
            p[[0, n // 2, n - 1]] = 0
        _POINTS[n] = p
    return _POINTS[n]


def _scaled_host(n, xname):
    if (n, xname) not in _SCALED:
        _SCALED[n, xname] = _cer().scale_g1(None, _points(n), _x(xname))
    return _SCALED[n, xname]


@pytest.mark.parametrize('xname', ['one', 'two', 'r_minus_1', 'random', 'naf255'])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_scale_kernel_equals_the_host_entry(ctx, oracle, n, xname):
    pts, want = _points(n), _scaled_host(n, xname)
    with _Dev(ctx, pts) as d_in, _Dev(ctx, np.full((n, 64), 0xa5, np.uint8)) as d_out:
        _cer().scale_g1_dev(ctx, d_in.ptr, n, _x(xname), d_out.ptr)                 # out of place
        assert d_out.get((n, 64)).tobytes() == want.tobytes()
        assert d_in.get((n, 64)).tobytes() == pts.tobytes()
        _cer().scale_g1_dev(ctx, d_in.ptr, n, _x(xname), d_in.ptr)                  # in place
        assert d_in.get((n, 64)).tobytes() == want.tobytes()
    assert _cer().scale_g1(ctx, pts, _x(xname)).tobytes() == want.tobytes()          # host buffers through the kernel
    if n >= 3:
        assert not want[[0, n // 2, n - 1]].any() and want[1].any()
    for i in sorted({1, n // 3, n - 2} & set(range(n))):                            # a handful against the oracle
        assert want[i].tobytes() == oracle.g1_mul(pts[i], _x(xname)).tobytes(), i


def test_scale_by_zero_gives_infinity_everywhere(ctx):
    assert not _cer().scale_g1(ctx, _points(65), fx.mont_fr(0)).any()


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 1025])
def test_weights_kernel_equals_the_host_entry(ctx, n):
    got = _cer().weights(cc.SEED, n, ctx=ctx)
    assert got.shape == (n, 4) and got.tobytes() == _cer().weights(cc.SEED, n).tobytes()


_PROOFS = {}


def _oracle_proof(oracle, c, key, tag):
    """the oracle's proof of case c under `key` (r, s fixed), once per session"""
    if tag not in _PROOFS:
        z = fx.witness_mont(c.z_in, c.z_aux)
        a, b, cc_, aa, bi, ba = oracle.synthesize(c.csr, z)
        r, s = fx.mont_fr(0xace), fx.mont_fr(0xbee)
        _PROOFS[tag] = ((a, b, cc_, z, aa, bi, ba, r, s), oracle.prove(key, a, b, cc_, z, aa, bi, ba, r, s).tobytes())
    return _PROOFS[tag]


@pytest.mark.parametrize('levels', [False, True])
@pytest.mark.parametrize('shape,unused,xname', [('tiny', False, 'random'), ('tiny', True, 'two'), ('small', False, 'random'), ('small', False, 'r_minus_1'),
                                                ('mid', False, 'random'), ('big', False, 'random')])
def test_contribution_is_the_oracles_setup_with_delta_x(ctx, oracle, shape, unused, xname, levels):
    c = cc.case(shape, unused)
    x = cc.XS[xname]
    dk = ctx.load_key(c.params)
    new, deltas = _cer().contribute(ctx, dk, _x(xname), levels=levels)
    got = {n: new.download(n) for n in ('h', 'l', 'a', 'b_g1', 'b_g2')}
    got.update(new.vk())
    assert got['delta_g1'].tobytes() == deltas['delta_g1'].tobytes() and got['delta_g2'].tobytes() == deltas['delta_g2'].tobytes()
    cc.assert_contributed(got, c, x)
    if unused:
        assert not got['l'][-1].any()
    assert new.counts() == dk.counts()
    # the contributed key proves what the oracle proves with its delta x key ...
    want = c.expected(x)
    args, want_proof = _oracle_proof(oracle, c, want, (shape, unused, xname))
    proof = ctx.prove_raw(new, *args).tobytes()
    assert proof == want_proof
    if not levels:
        P = ref.proof_from_borsh(proof)
        assert ref.verify(fx.key_to_py(want), c.z_in[1:], P)
        assert not ref.verify(fx.key_to_py(c.key), c.z_in[1:], P)
    # ... and the input key still proves its old bytes
    _, old_proof = _oracle_proof(oracle, c, c.key, (shape, unused, None))
    assert ctx.prove_raw(dk, *args).tobytes() == old_proof
    for name in ('h', 'l'):
        assert dk.download(name).tobytes() == np.array(getattr(c.key, name)).tobytes()
    new.free(); dk.free()


def _same_report(dev, host):
    assert dev.flags() == host.flags() and dev.key_accept == host.key_accept and dev.delta_changed == host.delta_changed
    assert (dev.s_h, dev.s_h_after, dev.s_l, dev.s_l_after, dev.seed) == (host.s_h, host.s_h_after, host.s_l, host.s_l_after, host.seed)


@pytest.fixture(scope='module')
def keys(ctx):
    """shape -> (case, the oracle's key for delta * x as Parameters, the two resident keys), loaded once and freed with the module"""
    held = {}

    def get(shape):
        if shape not in held:
            c = cc.case(shape)
            after = c.expected_params(cc.XS['random'])
            held[shape] = (c, after, ctx.load_key(c.params), ctx.load_key(after))
        return held[shape]
    yield get
    for _, _, dk_before, dk_after in held.values():
        dk_before.free(); dk_after.free()


@pytest.mark.parametrize('kind', (None,) + cc.TAMPERS)
@pytest.mark.parametrize('shape', ['tiny', 'small', 'mid'])
def test_check_report_equals_the_host_reference(ctx, oracle, keys, shape, kind):
    c, after, dk_before, dk_after = keys(shape)
    if kind is None:
        bad, dk_bad = after, dk_after
    else:
        bad = cc.tamper(c, after, kind, cc.XS['random'])
        dk_bad = ctx.load_key(bad)
    rep = _cer().check(ctx, dk_before, dk_bad, cc.SEED)
    assert rep.flags() == cc.expect_flags(kind) and rep.accept is (kind is None)
    _same_report(rep, _cer().check_host(c.params, bad, cc.SEED))
    if kind is not None:
        dk_bad.free()


@pytest.mark.parametrize('kind', [None, 'h_mid', 'l_double'])
def test_check_on_many_workgroups(ctx, oracle, keys, kind):
    """m = 2^14: expected flags only (the host reference is slow there)"""
    c, after, dk_before, dk_after = keys('big')
    dk_bad = dk_after if kind is None else ctx.load_key(cc.tamper(c, after, kind, cc.XS['random']))
    rep = _cer().check(ctx, dk_before, dk_bad, cc.SEED)
    assert rep.flags() == cc.expect_flags(kind) and rep.accept is (kind is None)
    if kind is not None:
        dk_bad.free()


def test_check_draws_its_own_seed(ctx, oracle, keys):
    c, after, dk_before, dk_after = keys('small')
    r1, r2 = _cer().check(ctx, dk_before, dk_after), _cer().check(ctx, dk_before, dk_after)
    assert r1.accept and r2.accept and r1.seed != r2.seed and r1.s_h != r2.s_h
    _same_report(_cer().check(ctx, dk_before, dk_after, r1.seed), r1)            # a report can be reproduced from its seed


def test_device_contribution_passes_the_device_check(ctx, oracle, keys):
    c, after, dk_before, dk_after = keys('mid')
    new, _ = _cer().contribute(ctx, dk_before)                                   # x drawn and forgotten
    rep = _cer().check(ctx, dk_before, new)
    assert rep.accept and rep.delta_changed
    new.free()


def _image(c):
    from fawkes_crypto_amd import params_io as pio
    k = c.key
    arrays = dict(alpha_g1=k.alpha_g1, beta_g1=k.beta_g1, beta_g2=k.beta_g2, gamma_g2=k.gamma_g2, delta_g1=k.delta_g1, delta_g2=k.delta_g2,
                  ic=np.array(k.ic), h=np.array(k.h), l=np.array(k.l), a=np.array(k.a), b_g1=np.array(k.b_g1), b_g2=np.array(k.b_g2))
    return pio.store_parameters(arrays, c.r1cs, const_tracker_bits=[True, False, True])


def test_image_to_image(ctx, oracle):
    from fawkes_crypto_amd import params_io as pio
    c = cc.case('small')
    x = cc.XS['random']
    image = _image(c)
    new_image = _cer().contribute_image(ctx, image, _x('random'))
    assert isinstance(new_image, bytes) and len(new_image) == len(image)
    # the result is a Parameters image: it loads with the point checks, and holds the oracle's key for delta x
    key, dr, hdr = pio.load_parameters(ctx, new_image, checked=True, warm=False)
    got = {n: key.download(n) for n in ('h', 'l', 'a', 'b_g1', 'b_g2')}
    got.update(key.vk())
    cc.assert_contributed(got, c, x)
    assert hdr['const_tracker'] == [True, False, True] and hdr['gamma_g2'].tobytes() == c.key.gamma_g2.tobytes() and hdr['ic'].tobytes() == np.array(c.key.ic).tobytes()
    dr.free(); key.free()
    rep = _cer().check_image(ctx, image, new_image)
    assert rep.accept and rep.header_equal and rep.vk_equal and rep.flags() == cc.expect_flags()
    # another gate blob / another ic: the key part still passes, the image does not
    h0, h1 = pio.read_parameters(image), pio.read_parameters(new_image)
    other_header = pio.write_parameters(h1['num_gates'], bytes(h1['gates_blob']), [True, True, True], bytes(h1['bellman']))
    rep = _cer().check_image(ctx, image, other_header, cc.SEED)
    assert rep.key_accept and rep.header_equal is False and rep.vk_equal is True and rep.accept is False
    blob = bytearray(h1['gates_blob'])
    blob[len(blob) // 2] ^= 1
    rep = _cer().check_image(ctx, image, pio.write_parameters(h1['num_gates'], bytes(blob), h1['const_tracker'], bytes(h1['bellman'])), cc.SEED)
    assert rep.key_accept and rep.header_equal is False and rep.accept is False
    bell = bytearray(h1['bellman'])
    ic_at = 64 + 64 + 128 + 128 + 64 + 128 + 4          # the first ic point: swap it for the second
    bell[ic_at:ic_at + 64], bell[ic_at + 64:ic_at + 128] = bell[ic_at + 64:ic_at + 128], bell[ic_at:ic_at + 64]
    rep = _cer().check_image(ctx, image, pio.write_parameters(h1['num_gates'], bytes(h1['gates_blob']), h1['const_tracker'], bytes(bell)), cc.SEED)
    assert rep.key_accept and rep.header_equal is True and rep.vk_equal is False and rep.accept is False
    assert bytes(h0['gates_blob']) == bytes(h1['gates_blob'])


def test_guards(ctx, oracle, keys):
    from fawkes_crypto_amd import FkError
    cer = _cer()
    c, after, dk_before, dk_after = keys('small')

    def refused(fn, code=1):
        with pytest.raises(FkError) as e:
            fn()
        assert e.value.code == code

    refused(lambda: cer.contribute(ctx, dk_before, fx.mont_fr(0)))
    not_below_r = np.frombuffer(int(cc.R).to_bytes(32, 'little'), np.uint64).copy()
    refused(lambda: cer.contribute(ctx, dk_before, not_below_r), 7)
    refused(lambda: cer.scale_g1(ctx, _points(3), not_below_r), 7)
    shard = ctx.load_key(c.params, 0, 2)
    refused(lambda: cer.contribute(ctx, shard, _x('two')))
    refused(lambda: cer.check(ctx, shard, dk_after, cc.SEED))
    refused(lambda: cer.check(ctx, dk_before, shard, cc.SEED))
    shard.free()
    # a proof that holds the lanes between two calls
    dr = ctx.load_r1cs(c.r1cs)
    z = fx.witness_mont(c.z_in, c.z_aux)
    with _Dev(ctx, z) as d_z, _Dev(ctx, np.zeros((c.params.m, 4), np.uint64)) as d_h:
        ctx.prove_msms_z_begin_dev(dk_before, d_z.ptr, *dr.density_ptrs())
        try:
            refused(lambda: cer.contribute(ctx, dk_before, _x('two')))
            refused(lambda: cer.check(ctx, dk_before, dk_after, cc.SEED))
        finally:
            ctx.prove_msms_finish_dev(dk_before, d_h.ptr)
        assert cer.check(ctx, dk_before, dk_after, cc.SEED).accept
    dr.free()
