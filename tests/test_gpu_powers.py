"""Phase 1 of the key ceremony on the device (include/fawkes_hip_powers.h through fawkes_crypto_amd/powers.py): the scale kernel against the
oracle's g1_mul / g2_mul of scalars computed in Python -- sizes around the wave, the 64-bit exponent, short scalars, alternating signs,
infinity in edge lanes, in place --, a contribution against transcripts MADE BY THE ORACLE and against the host entry, the chain
contribute -> initial key against the oracle's setup, the point classes against the host report with planted points of every class, the
update check's report against the host reference for the honest update and every tamper, and the refusal beside a proof that holds the
lanes.  Every comparison is exact; nothing expected comes from the code under test.  A bad coordinate is only arithmetic."""
import numpy as np
import pytest

import bn254_ref as ref
import c_oracle as co
import ceremony_init_cases as ic
import fawkes_crypto_amd as fk
import fixtures as fx
import powers_cases as pc
from fawkes_crypto_amd import powers as PW

pytestmark = pytest.mark.gpu

R = ref.R
SIZES = (1, 63, 64, 65, 130)
GROUPS = dict(g1=(co.g1_mul, ic.g1, 64), g2=(co.g2_mul, ic.g2, 128))


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


_POINTS = {}


def _points(group, n=130):
    """n distinct oracle points of the group, made once"""
    if group not in _POINTS:
        gen = GROUPS[group][1]
        _POINTS[group] = np.array([gen(0x51ed + 7 * i) for i in range(max(SIZES))])
    return _POINTS[group][:n]


def _want(group, pts, x, c, first):
    mul = GROUPS[group][0]
    return np.array([mul(pts[i], pc.mont(c * pow(x, first + i, R))) if pts[i].any() else pts[i] for i in range(pts.shape[0])])


# ---------------------------------------------------------------- the scale kernel
@pytest.mark.parametrize('first', [0, 5, (1 << 32) + 5])
@pytest.mark.parametrize('group', ['g1', 'g2'])
def test_scale_kernel_sizes_and_offset(ctx, oracle, group, first):
    for n in SIZES:
        pts = _points(group, n)
        got = fk.scale_powers(ctx, pts, pc.mont(pc.X), pc.mont(pc.Y), first=first)
        assert got.tobytes() == _want(group, pts, pc.X, pc.Y, first).tobytes(), n


@pytest.mark.parametrize('c', [1, pc.Z])
@pytest.mark.parametrize('x', [1, 2, R - 1, pc.X])
@pytest.mark.parametrize('group', ['g1', 'g2'])
def test_scale_kernel_scalars(ctx, oracle, group, x, c):
    pts = _points(group, 65)
    got = fk.scale_powers(ctx, pts, pc.mont(x), None if c == 1 else pc.mont(c), first=0)
    assert got.tobytes() == _want(group, pts, x, c, 0).tobytes()
    if x == R - 1 and c == 1:          # alternating signs: the point itself, then its negative
        add = co.g1_add if group == 'g1' else co.g2_add
        assert got[0].tobytes() == pts[0].tobytes() and got[1].tobytes() != pts[1].tobytes() and not add(got[1], pts[1]).any()


@pytest.mark.parametrize('group', ['g1', 'g2'])
def test_scale_kernel_edge_lanes_and_entry_points(ctx, oracle, group):
    width = GROUPS[group][2]
    pts = _points(group, 130).copy()
    for i in (0, 64, 129):             # infinity in the first, a middle and the last lane
        pts[i] = 0
    x, c, first = pc.mont(pc.X), pc.mont(pc.Z), 3
    want = _want(group, pts, pc.X, pc.Z, first)
    got = fk.scale_powers(ctx, pts, x, c, first=first)
    assert got.tobytes() == want.tobytes() and not got[[0, 64, 129]].any()
    assert got.tobytes() == fk.scale_powers(None, pts, x, c, first=first).tobytes(), 'device against the host entry'
    with _Dev(ctx, pts) as d_in, _Dev(ctx, np.zeros_like(pts)) as d_out:
        fk.scale_powers_dev(ctx, d_in.ptr, 130, x, c, first, d_out.ptr, g2=group == 'g2')          # out of place: the input stays
        assert d_out.get((130, width)).tobytes() == want.tobytes() and d_in.get((130, width)).tobytes() == pts.tobytes()
        fk.scale_powers_dev(ctx, d_in.ptr, 130, x, c, first, d_in.ptr, g2=group == 'g2')           # in place
        assert d_in.get((130, width)).tobytes() == want.tobytes()


# ---------------------------------------------------------------- contribute
@pytest.mark.parametrize('m', [2, 4, 64, 128])
def test_contribute_is_the_oracles_transcript(ctx, oracle, m):
    first, pub1 = fk.contribute(ctx, fk.new_powers(m), pc.mont(pc.TAU), pc.mont(pc.ALPHA), pc.mont(pc.BETA))
    pc.same_transcript(first, pc.before(m))
    assert (pub1.x_g2.tobytes(), pub1.y_g2.tobytes(), pub1.z_g2.tobytes()) == (pc.g2(pc.TAU).tobytes(), pc.g2(pc.ALPHA).tobytes(), pc.g2(pc.BETA).tobytes())
    src = pc.before(m)
    second, pub2 = fk.contribute(ctx, src, pc.mont(pc.X), pc.mont(pc.Y), pc.mont(pc.Z))
    pc.same_transcript(second, pc.after(m))
    want = pc.public()
    assert (pub2.x_g2.tobytes(), pub2.y_g2.tobytes(), pub2.z_g2.tobytes()) == (want.x_g2.tobytes(), want.y_g2.tobytes(), want.z_g2.tobytes())
    if m <= 8:
        host, pub_h = fk.contribute_host(src, pc.mont(pc.X), pc.mont(pc.Y), pc.mont(pc.Z))
        pc.same_transcript(second, host)
        assert pub2.x_g2.tobytes() == pub_h.x_g2.tobytes()


def test_chain_contribute_then_initial_key(ctx, oracle):
    c = ic.case('small')
    assert c.m == 64
    pw, _ = fk.contribute(ctx, pc.before(64), pc.mont(pc.X), pc.mont(pc.Y), pc.mont(pc.Z))
    p = fk.initial_key(ctx, pw, c.r1cs)
    try:
        want = co.setup(c.csr, pc.TAU * pc.X % R, pc.ALPHA * pc.Y % R, pc.BETA * pc.Z % R, 1, 1)
        ic.assert_key(dict(h=p.h, l=p.l, a=p.a, b_g1=p.b_g1, b_g2=p.b_g2), p.vk_full, p.ic, want)
    finally:
        p.key.free()


# ---------------------------------------------------------------- validate points
@pytest.mark.parametrize('group', ['g1', 'g2'])
def test_validate_points_equals_the_host_report(ctx, oracle, group):
    pts = _points(group, 130).copy()
    assert fk.validate_points(ctx, pts) == fk.validate_points(None, pts) and fk.validate_points(ctx, pts).ok
    classes = pc.CLASSES[group]
    # two bad points per class: at the first, a middle and the last index, and three more inside
    where = [0, 64, 129, 1, 63, 65, 100, 128][:2 * len(classes)]
    for k, i in enumerate(where):
        pts[i] = pc.bad_point(group, classes[k % len(classes)], salt=k)
    rep = fk.validate_points(ctx, pts)
    assert rep.counts() == {c: (2 if c in classes else 0) for c in ('infinity', 'range', 'curve', 'subgroup')} and rep.first_bad == 0
    assert rep == fk.validate_points(None, pts)
    rep = fk.validate_points(ctx, pts[66:128])           # the only bad point of this piece: index 100 - 66
    want_cls = classes[where.index(100) % len(classes)] if 100 in where else None
    if want_cls is None:
        assert rep.ok and rep.first_bad is None
    else:
        assert rep.counts()[want_cls] == 1 and sum(rep.counts().values()) == 1 and rep.first_bad == 34
    assert rep == fk.validate_points(None, pts[66:128])
    with _Dev(ctx, pts) as d_pts, _Dev(ctx, np.zeros(5, np.uint64)) as d_rep:          # the asynchronous entry: points and report on the device
        PW.validate_points_dev(ctx, d_pts.ptr, 130, group == 'g2', d_rep.ptr)
        raw = d_rep.get((40,)).view(np.uint64)
        assert [int(v) for v in raw] == [2, 2, 2, 2 if group == 'g2' else 0, 0]


# ---------------------------------------------------------------- check an update
def _same_report(dev, host):
    assert dev.flags() == host.flags() and dev.accept == host.accept and dev.changed == host.changed
    assert dev.points == host.points
    assert dev.after.flags() == host.after.flags() and dev.after.accept == host.after.accept
    assert dev.after.sums() == host.after.sums() and dev.after.seed == host.after.seed


@pytest.mark.parametrize('kind', (None,) + pc.TAMPERS)
def test_update_check_equals_the_host_reference(ctx, oracle, kind):
    b, a, p = pc.tampered(64, kind)
    rep = fk.check_update(ctx, b, a, p, 64, pc.SEED)
    pc.assert_update_report(rep, 64, kind)
    _same_report(rep, fk.check_update_host(b, a, p, 64, pc.SEED))


def test_update_check_draws_its_own_seed(ctx, oracle):
    b, a, p = pc.tampered(64, None)
    r1, r2 = fk.check_update(ctx, b, a, p, 64), fk.check_update(ctx, b, a, p, 64)
    assert r1.accept and r2.accept and r1.after.seed != r2.after.seed
    _same_report(fk.check_update(ctx, b, a, p, 64, r1.after.seed), r1)


# ---------------------------------------------------------------- guards
def test_refusals_beside_a_proof_that_holds_the_lanes(ctx, oracle):
    c = ic.case('small')
    b, a, p = pc.tampered(64, None)
    x = pc.mont(pc.X)

    def refused(fn, code=1):
        with pytest.raises(fk.FkError) as e:
            fn()
        assert e.value.code == code

    refused(lambda: fk.contribute(ctx, b, np.zeros(4, np.uint64), x, x))
    params = fk.initial_key(ctx, ic.transcript(), c.r1cs)
    dk = params.key
    dr = ctx.load_r1cs(c.r1cs)
    z = fx.witness_mont(c.z_in, c.z_aux)
    with _Dev(ctx, z) as d_z, _Dev(ctx, np.zeros((c.m, 4), np.uint64)) as d_h:
        ctx.prove_msms_z_begin_dev(dk, d_z.ptr, *dr.density_ptrs())
        try:
            refused(lambda: fk.contribute(ctx, b, x, x, x))
            refused(lambda: fk.check_update(ctx, b, a, p, 64, pc.SEED))
            refused(lambda: fk.scale_powers(ctx, b.tau_g1, x))
            refused(lambda: fk.validate_points(ctx, b.tau_g1))
        finally:
            ctx.prove_msms_finish_dev(dk, d_h.ptr)
    # the context is still usable
    assert fk.check_update(ctx, b, a, p, 64, pc.SEED).accept
    got, _ = fk.contribute(ctx, pc.before(4), x, pc.mont(pc.Y), pc.mont(pc.Z))
    pc.same_transcript(got, pc.after(4))
    dr.free(); dk.free()
