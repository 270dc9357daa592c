"""The batch prover's R1CS check on the GPU (include/fawkes_hip_batch_check.h).  The stage entry fk_batch_r1cs_check_dev must equal the
host entry fk_batch_r1cs_check on every output (tests/test_batch_check_host.py holds that one to the oracle): wave, word and block edges,
both witness layouts, several groups, guard words around the device arrays.  The checked prover must return the unchecked prover's bytes
and the host entry's reports, and the chained call must flag exactly the given row that is wrong.  Every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc
import fixtures as fx
import witness_trace
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import batch as B
from fawkes_crypto_amd import check as K
from fawkes_crypto_amd import witness as W
from batch_cases import tile_rows
from batch_check_cases import GATES, LAYOUTS, laid_out, range_cases, range_system, variants
from helpers import params_from_oracle_key, r1cs_product, TOXIC
import check_cases as cc

pytestmark = pytest.mark.gpu
R = ref.R
COUNTS = (1, 3, 65)
GUARD, GUARD_WORDS, GUARD_BYTES = 0xa5a5a5a5a5a5a5a5, 4, 16


class Dev:
    """device arrays of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.dev_alloc(max(arr.nbytes, 32))
        self.ptrs.append(p)
        if arr.nbytes:
            self.ctx.upload(p, arr)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.dev_free(p)


def host(prod, z, layout, count):
    """fk_batch_r1cs_check: (report fields per proof, bitmap bytes, flag bytes)"""
    words = (prod.num_gates + 63) // 64
    bitmap, flags = np.zeros(count * words, np.uint64), np.zeros(count, np.uint8)
    sts = (K.CheckReportStruct * count)()
    assert B._lib().fk_batch_r1cs_check(None, C.byref(prod.struct), z.ctypes.data, layout, count, bitmap.ctypes.data, flags.ctypes.data, sts) == 0
    return [cc.struct_fields(st) for st in sts], bitmap.tobytes(), flags.tobytes()


class Guarded:
    """the device bitmap and flags of `count` proofs between guard words, which no call may touch"""

    def __init__(self, dev, gates, count):
        self.ctx, self.count, self.words = dev.ctx, count, (gates + 63) // 64
        self.d_bitmap = dev.put(np.full(count * self.words + 2 * GUARD_WORDS, GUARD, np.uint64))
        self.d_flags = dev.put(np.full(count + 2 * GUARD_BYTES, 0x5a, np.uint8))
        self.bitmap, self.flags = self.d_bitmap + 8 * GUARD_WORDS, self.d_flags + GUARD_BYTES

    def read(self):
        """(bitmap bytes, flag bytes), the guards checked"""
        bm = self.ctx.download(self.d_bitmap, 8 * (self.count * self.words + 2 * GUARD_WORDS), np.uint64)
        fl = self.ctx.download(self.d_flags, self.count + 2 * GUARD_BYTES, np.uint8)
        assert (bm[:GUARD_WORDS] == GUARD).all() and (bm[-GUARD_WORDS:] == GUARD).all(), 'the bitmap was written outside its extent'
        assert (fl[:GUARD_BYTES] == 0x5a).all() and (fl[-GUARD_BYTES:] == 0x5a).all(), 'the flags were written outside their extent'
        return bm[GUARD_WORDS:-GUARD_WORDS].tobytes(), fl[GUARD_BYTES:-GUARD_BYTES].tobytes()


def device(ctx, dr, d_z, layout, count, out, opts=None):
    """fk_batch_r1cs_check_dev into guarded arrays: the same triple as host()"""
    sts = (K.CheckReportStruct * count)()
    ctx._ck(B._lib().fk_batch_r1cs_check_dev(ctx.handle, dr.handle, d_z, layout, count, out.bitmap, out.flags, sts, B._opts(opts)))
    return ([cc.struct_fields(st) for st in sts],) + out.read()


@pytest.fixture(scope='module')
def resident(ctx):
    """gates -> the explicit system of that many gates on the device, loaded once"""
    held = {}

    def get(gates):
        if gates not in held:
            held[gates] = ctx.load_r1cs(variants(gates)[1])
        return held[gates]

    yield get
    for dr in held.values():
        dr.free()


def patterns(var, count):
    """name -> which variant each proof holds.  var[0] satisfies, var[1] breaks gate 0, var[-1] every gate; where the system has them,
    var[3] breaks gates 63 and 64"""
    straddle = 3 if len(var) > 4 else len(var) - 2
    last = count - 1
    out = {'none': {}, 'proof 0 only': {0: 1}, 'the last proof only': {last: 1}, 'all gates of one proof': {count // 2: len(var) - 1},
           '63 and 64 in one proof, 0 in another': {last: straddle, 0: 1} if count > 1 else {0: straddle}}
    return {name: [var[at.get(i, 0)][0] for i in range(count)] for name, at in out.items()}


# ---------------------------------------------------------------- the stage entry
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('gates', GATES)
def test_stage_entry_equals_the_host_entry(ctx, oracle, resident, gates, count, layout):
    csr, prod, var = variants(gates)
    if gates > 64:
        assert cc.bad_sets(gates)[2] == [63, 64]
    dr = resident(gates)
    for name, zs in patterns(var, count).items():
        z = laid_out(zs, layout, csr.num_input)
        want = host(prod, z, layout, count)
        if name != 'none':
            assert any(f['n_bad'] for f in want[0]) and 1 in want[2]
        with Dev(ctx) as d:
            d_z, out = d.put(z), Guarded(d, gates, count)
            got = device(ctx, dr, d_z, layout, count, out)
            assert got == want, (gates, count, layout, name)
            assert device(ctx, dr, d_z, layout, count, out) == got, 'the call made twice differs'


@pytest.mark.parametrize('layout', LAYOUTS)
def test_several_groups_with_a_short_last_one(ctx, oracle, resident, layout):
    """257 gates x 65 proofs under a budget of 30 proofs: groups of 30, 30 and 5.  The bad proofs are the first and the last of every
    group, so a group's first-proof offset (witness, bitmap, flags, reports) and the tiled order's `count` both show."""
    gates, count, group = 257, 65, 30
    csr, prod, var = variants(gates)
    dr = resident(gates)
    m = 1 << (dr.info()['rows'] - 1).bit_length()
    budget = group * (3 * m * 32 + B.CHECK_RECORD_BYTES)
    bad = {0: 1, 29: 2, 30: 3, 59: len(var) - 1, 60: 4, 64: 1}
    zs = [var[bad.get(i, 0)][0] for i in range(count)]
    z = laid_out(zs, layout, csr.num_input)
    want = host(prod, z, layout, count)
    assert [i for i, f in enumerate(want[0]) if f['n_bad']] == sorted(bad)
    with Dev(ctx) as d:
        d_z, out = d.put(z), Guarded(d, gates, count)
        assert device(ctx, dr, d_z, layout, count, out, dict(scratch_budget_bytes=budget)) == want
        assert device(ctx, dr, d_z, layout, count, out, dict(scratch_budget_bytes=budget + 1)) == want
        assert device(ctx, dr, d_z, layout, count, out, dict(scratch_budget_bytes=1)) == want             # groups of one
        assert device(ctx, dr, d_z, layout, count, out) == want                                          # one group


def test_range_and_one(ctx, oracle):
    csr, prod, z = range_system()
    dr = ctx.load_r1cs(prod)
    for (name, layout), (zs, expect) in range_cases(csr, z).items():
        zl = laid_out(zs, layout, csr.num_input)
        want = host(prod, zl, layout, 3)
        with Dev(ctx) as d:
            got = device(ctx, dr, d.put(zl), layout, 3, Guarded(d, csr.num_gates, 3))
        for i, (zi, e) in enumerate(zip(zs, expect)):         # the judged proofs also straight against the oracle: the neighbour of an unjudged proof stays exact
            assert got[0][i] == (cc.want_fields(cc.Want(csr, zi)) if e is None else e), (name, layout, i)
        assert got == want, (name, layout)
    dr.free()


def test_python_wrappers_of_the_stage_entry(ctx, oracle, resident):
    csr, prod, var = variants(65)
    dr = resident(65)
    zs = np.stack([x for x, _ in var])
    reps = B.check_batch(ctx, dr, zs)
    assert len(reps) == len(var)
    for rep, (_, w) in zip(reps, var):
        cc.assert_report(rep, w)
    with Dev(ctx) as d:
        reps = B.check_batch_dev(ctx, dr, d.put(tile_rows(list(zs), csr.num_input)), B.Z_TILED, len(var), opts=dict(scratch_budget_bytes=1))
    for rep, (_, w) in zip(reps, var):
        cc.assert_report(rep, w)
    assert B.check_batch(ctx, dr, zs[:0]) == []


# ---------------------------------------------------------------- checked proving
@pytest.fixture(scope='module')
def small(ctx, oracle):
    """900 gates, five witnesses of which four are violated (tests/test_gpu_batch_prove.py: `small`)"""
    cs, z_in, z_aux = ref.random_r1cs(77, 900, 3, 950)
    csr = fx.r1cs_to_csr(cs)
    prod = r1cs_product(csr)
    key = oracle.setup(csr, **TOXIC)
    params = params_from_oracle_key(key, prod)
    dk, dr = ctx.load_key(params), ctx.load_r1cs(params.r1cs)
    rnd = random.Random(12)
    auxs = [list(z_aux)]
    for k in range(3):
        a = list(z_aux)
        for j in rnd.sample(range(len(a)), 5 + k):
            a[j] = rnd.randrange(R)
        auxs.append(a)
    auxs.append([1] * len(z_aux))
    zs = np.stack([fx.witness_mont(z_in, a) for a in auxs])
    rs = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in auxs])
    ss = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in auxs])
    single = [ctx.prove_witness(dk, dr, zs[i], rs[i], ss[i]).tobytes() for i in range(5)]
    unchecked = B.prove_batch(ctx, dk, dr, zs, rs, ss)
    rows = np.ascontiguousarray(zs.reshape(-1, 4))
    want = {B.Z_ROWS: host(prod, rows, B.Z_ROWS, 5), B.Z_TILED: host(prod, tile_rows(list(zs), 3), B.Z_TILED, 5)}
    assert want[B.Z_ROWS] == want[B.Z_TILED] and [f['n_bad'] > 0 for f in want[B.Z_ROWS][0]] == [False, True, True, True, True]
    yield dict(csr=csr, prod=prod, params=params, dk=dk, dr=dr, zs=zs, rs=rs, ss=ss, single=single, unchecked=unchecked, want=want[B.Z_ROWS])
    dr.free(); dk.free()


def checked_raw(ctx, s, d_z, layout, opts=None, host_z=None):
    """fk_prove_batch_checked_dev (or, with host_z, fk_prove_batch_checked) into guarded arrays: (proof bytes, (fields, bitmap, flags), check_ms)"""
    proofs, sts, ms = np.zeros((5, 256), np.uint8), (K.CheckReportStruct * 5)(), C.c_double(-1)
    lib = B._lib()
    with Dev(ctx) as d:
        out = Guarded(d, s['csr'].num_gates, 5)
        tail = (s['rs'].ctypes.data, s['ss'].ctypes.data, proofs.ctypes.data, B._opts(opts), None, out.bitmap, out.flags, sts, C.byref(ms))
        if host_z is None:
            ctx._ck(lib.fk_prove_batch_checked_dev(ctx.handle, s['dk'].handle, s['dr'].handle, d_z, layout, 5, *tail))
        else:
            ctx._ck(lib.fk_prove_batch_checked(ctx.handle, s['dk'].handle, s['dr'].handle, host_z.ctypes.data, 5, *tail))
        return [p.tobytes() for p in proofs], ([cc.struct_fields(st) for st in sts],) + out.read(), ms.value


def test_checked_prover_gives_the_unchecked_bytes_and_the_host_reports(ctx, small):
    s = small
    dk, dr, zs, rs, ss = s['dk'], s['dr'], s['zs'], s['rs'], s['ss']
    assert [p.tobytes() for p in s['unchecked']] == s['single'] and len(set(s['single'])) == 5
    c = dk.counts()
    two = B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], 2, dict(scratch_budget_bytes=1 << 40))['scratch_bytes']
    assert (lambda p: (p['group'], p['n_groups']))(B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], 5, dict(scratch_budget_bytes=two))) == (2, 3)
    with Dev(ctx) as d:
        d_z = {B.Z_ROWS: d.put(zs), B.Z_TILED: d.put(tile_rows(list(zs), 3))}
        for layout in LAYOUTS:
            for opts in (None, dict(scratch_budget_bytes=two)):           # one group; groups of 2, 2, 1
                proofs, verdicts, ms = checked_raw(ctx, s, d_z[layout], layout, opts)
                assert proofs == s['single'], (layout, opts)
                assert verdicts == s['want'], (layout, opts)
                assert ms > 0, (layout, opts)
        # the host-witness entry
        proofs, verdicts, ms = checked_raw(ctx, s, None, B.Z_ROWS, dict(scratch_budget_bytes=two), host_z=np.ascontiguousarray(zs))
        assert proofs == s['single'] and verdicts == s['want'] and ms > 0
        # an unchecked call right behind gives unchanged bytes
        assert B.prove_batch_dev(ctx, dk, dr, d_z[B.Z_TILED], B.Z_TILED, 5, rs, ss).tobytes() == s['unchecked'].tobytes()
    assert B.prove_batch(ctx, dk, dr, zs, rs, ss).tobytes() == s['unchecked'].tobytes()


def test_checked_prover_wrappers_timings_trim_and_raise_on_bad(ctx, small):
    s = small
    dk, dr, zs, rs, ss = s['dk'], s['dr'], s['zs'], s['rs'], s['ss']
    host_reports = B.check_batch_host(s['prod'], zs)

    def same(reps):
        assert len(reps) == 5
        for rep, h, f in zip(reps, host_reports, s['want'][0]):
            assert (rep.gates, rep.n_bad, rep.first_bad, rep.n_range, rep.one_ok, rep.gates_valid, rep.ok) == (h.gates, h.n_bad, h.first_bad, h.n_range, h.one_ok, h.gates_valid, h.ok)
            assert rep.n_bad == f['n_bad'] and np.array_equal(rep.first_abc_mont, h.first_abc_mont)
            assert np.array_equal(rep.bitmap(), h.bitmap()) and np.array_equal(rep.bad_rows(), h.bad_rows()) and len(rep.bad_rows()) == rep.n_bad

    proofs, reps, tm = B.prove_batch_checked(ctx, dk, dr, zs, rs, ss, want_timings=True)
    assert proofs.tobytes() == s['unchecked'].tobytes()
    same(reps)
    assert [rep.ok for rep in reps] == [True, False, False, False, False]
    assert tm['check_ms'] > 0 and tm['total_ms'] > 0 and all(tm[k] > 0 for k in ('eval_ms', 'quotient_ms', 'msm_h_ms', 'assemble_ms'))
    # the scratch is the context's: trim releases it, the next call grows it again
    ctx.trim()
    proofs, reps = B.prove_batch_checked(ctx, dk, dr, zs, rs, ss)
    assert proofs.tobytes() == s['unchecked'].tobytes()
    same(reps)
    same(B.check_batch(ctx, dr, zs))
    # raise_on_bad: the indices, the reports and the proofs that were made anyway
    with pytest.raises(B.BatchUnsatisfied) as e:
        B.prove_batch_checked(ctx, dk, dr, zs, rs, ss, raise_on_bad=True)
    assert e.value.bad == [1, 2, 3, 4] and e.value.proofs.tobytes() == s['unchecked'].tobytes()
    same(e.value.reports)
    proofs, reps = B.prove_batch_checked(ctx, dk, dr, zs[:1], rs[:1], ss[:1], raise_on_bad=True)              # nothing bad: no exception
    assert proofs.tobytes() == s['unchecked'][:1].tobytes() and reps[0].ok
    assert B.prove_batch_checked(ctx, dk, dr, zs[:0], rs[:0], ss[:0])[1] == []


def test_checked_prover_refusals_leave_the_context_usable(ctx, small):
    s = small
    dk, dr, zs, rs, ss = s['dk'], s['dr'], s['zs'], s['rs'], s['ss']
    lib = B._lib()
    proofs, sts = np.zeros((5, 256), np.uint8), (K.CheckReportStruct * 5)()

    def refused(code, said, fn):
        with pytest.raises(fk.FkError) as e:
            fn()
        assert e.value.code == code and said in str(e.value), str(e.value)

    with Dev(ctx) as d:
        d_z = d.put(zs)
        head = (ctx.handle, dk.handle, dr.handle, d_z)
        io = (rs.ctypes.data, ss.ctypes.data, proofs.ctypes.data, None, None)
        refused(1, 'reports', lambda: ctx._ck(lib.fk_prove_batch_checked_dev(*head, B.Z_ROWS, 5, *io, None, None, None, None)))
        refused(1, 'reports', lambda: ctx._ck(lib.fk_batch_r1cs_check_dev(ctx.handle, dr.handle, d_z, B.Z_ROWS, 5, None, None, None, None)))
        refused(1, 'layout', lambda: B.prove_batch_checked_dev(ctx, dk, dr, d_z, 2, 5, rs, ss))
        refused(1, 'layout', lambda: B.check_batch_dev(ctx, dr, d_z, 2, 5))
        refused(1, 'null', lambda: B.prove_batch_checked_dev(ctx, dk, dr, None, B.Z_ROWS, 5, rs, ss))
        refused(1, 'null', lambda: B.check_batch_dev(ctx, dr, None, B.Z_ROWS, 5))
        assert not proofs.any() and bytes(sts) == bytes(C.sizeof(sts))
        # count == 0: FK_OK whatever else is null, nothing written
        assert lib.fk_prove_batch_checked_dev(ctx.handle, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None) == 0
        assert lib.fk_batch_r1cs_check_dev(ctx.handle, None, None, 0, 0, None, None, None, None) == 0
        # without a context
        assert lib.fk_prove_batch_checked_dev(None, *head[1:], B.Z_ROWS, 5, *io, None, None, sts, None) == 1
        assert lib.fk_batch_r1cs_check_dev(None, dr.handle, d_z, B.Z_ROWS, 5, None, None, sts, None) == 1
    tiled = ctx.load_r1cs(s['prod'], copies=2)
    refused(1, 'tiled', lambda: B.check_batch(ctx, tiled, np.zeros((2, tiled.info()['num_vars'], 4), np.uint64)))
    refused(1, 'tiled', lambda: B.prove_batch_checked(ctx, dk, tiled, np.zeros((2, tiled.info()['num_vars'], 4), np.uint64), rs[:2], ss[:2]))
    tiled.free()
    shard = ctx.load_key(s['params'], 0, 2)
    refused(1, 'sharded', lambda: B.prove_batch_checked(ctx, shard, dr, zs, rs, ss))
    shard.free()
    # between submit and wait: refused, and the waiting ticket still gives its own proof
    ticket = ctx.prove_witness_submit(dk, dr, np.ascontiguousarray(zs[1]), rs[1], ss[1])
    refused(1, 'outstanding', lambda: B.prove_batch_checked(ctx, dk, dr, zs, rs, ss))
    refused(1, 'outstanding', lambda: B.check_batch(ctx, dr, zs))
    assert ctx.prove_witness_wait(ticket).tobytes() == s['single'][1]
    # the context is as usable as before
    got, reps = B.prove_batch_checked(ctx, dk, dr, zs[:2], rs[:2], ss[:2])
    assert [g.tobytes() for g in got] == s['single'][:2] and [rep.ok for rep in reps] == [True, False]


# ---------------------------------------------------------------- from the given rows
_P3 = fc.PoseidonParams(3, 8, 53)


def _merkle_params(k):
    rnd = random.Random(100 + k)
    return rnd.randrange(R), [rnd.randrange(R) for _ in range(2)], [rnd.randrange(2) for _ in range(2)]


def test_prove_given_batch_checked_flags_exactly_the_wrong_given_row(ctx, oracle):
    """the depth-2 Merkle gadget of tests/test_gpu_batch_prove.py, traced once; three given rows, the middle one with a path bit flipped
    under the root of the true path"""
    with witness_trace.trace() as t:
        first = fc.poseidon_merkle_circuit(*_merkle_params(0), 2, _P3)[0]
    prog, g0 = t.program(first)
    given = [g0] + [[fc.poseidon_merkle_proof_root(leaf, sib, path, _P3), leaf, *sib, *path] for leaf, sib, path in (_merkle_params(k) for k in (1, 2))]
    given[1] = list(given[1])
    given[1][-1] = 1 - given[1][-1]
    csr = fx.r1cs_to_csr(first.r1cs())
    prod = r1cs_product(csr)
    key = oracle.setup(csr, **TOXIC)
    dk, dr = ctx.load_key(params_from_oracle_key(key, prod)), ctx.load_r1cs(prod)
    dp = W.load(ctx, prog)
    rs = np.stack([fx.mont_fr(0x5eed0 + i) for i in range(3)])
    ss = np.stack([fx.mont_fr(0xfeed0 + i) for i in range(3)])
    want = B.prove_given_batch(ctx, dp, dk, dr, given, rs, ss)
    got, reps = B.prove_given_batch_checked(ctx, dp, dk, dr, given, rs, ss)
    assert got.shape == (3, 256) and got.tobytes() == want.tobytes()
    assert [rep.ok for rep in reps] == [True, False, True]
    assert reps[1].n_bad > 0 and reps[1].gates_valid and reps[1].n_range == 0 and list(reps[1].bad_rows())[0] == reps[1].first_bad
    # the verdicts are the host entry's on the host run of the same program
    zs = np.stack([fk.api._fr_rows(prog.run_host([gv])) for gv in given])
    for rep, h in zip(reps, B.check_batch_host(prod, zs)):
        assert (rep.n_bad, rep.first_bad) == (h.n_bad, h.first_bad) and np.array_equal(rep.bitmap(), h.bitmap())
    vk = fx.key_to_py(key)
    for i in range(3):
        assert ref.verify(vk, [int(given[i][0])], ref.proof_from_borsh(got[i].tobytes())) == (i != 1), i
    with pytest.raises(B.BatchUnsatisfied) as e:
        B.prove_given_batch_checked(ctx, dp, dk, dr, given, rs, ss, raise_on_bad=True)
    assert e.value.bad == [1] and e.value.proofs.tobytes() == want.tobytes()
    dp.free(); dr.free(); dk.free()
