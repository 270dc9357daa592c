"""Repeated linear combinations are evaluated once (csrc/spmv.hip, the alias plan): a row whose columns and coefficient indices repeat an
earlier row's exactly is left out of spmv_binned_kernel's lists and copied from its source by spmv_alias_kernel.  The alias table the
library planned is compared EXACTLY with a restatement of the rule held here (`reference_aliases`), under the minimum length and the
look-back fk_r1cs_alias_info reports, and a, b, c with the oracle's `synthesize`, as tests/test_gpu_r1cs.py does.  The two inspection
entry points are test-only (include/fawkes_hip_inspect.h) and are called here through ctypes directly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_ref as ref
import fixtures as fx
from helpers import r1cs_product, TOXIC
from spmv_plan_cases import BIN_MIN, crafted_system, reference_aliases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alias_info(dr):
    out = (C.c_uint64 * 4)()
    fn = dr.ctx.lib.fk_r1cs_alias_info
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    assert fn(dr.handle, out) == 0
    return dict(zip(('aliases', 'terms', 'min', 'lookback'), (int(x) for x in out)))


def alias_table(dr):
    n = alias_info(dr)['aliases']
    arr = [np.zeros(max(n, 1), np.uint32) for _ in range(4)]
    fn = dr.ctx.lib.fk_r1cs_aliases
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
    assert fn(dr.handle, n, *[a.ctypes.data for a in arr]) == 0
    return [tuple(int(a[i]) for a in arr) for i in range(n)]          # (dst matrix, dst row, src matrix, src row)


def random_z(nv, seed):
    rnd = np.random.default_rng(seed)
    z = fx.co.limbs_arr([int(x) % ref.R for x in rnd.integers(1, 2**63, nv).astype(object) * (2**190 + 12345 + seed)])
    z[0] = fx.mont_fr(1)
    return z


def evaluate(ctx, dr, z, rows, sliced=None):
    """a, b, c of fk_r1cs_eval_dev (or of one cyclic slice: sliced = (log_m, rank, log_w)) over buffers filled with a marker"""
    m = 1 << max(rows - 1, 1).bit_length()
    d = [ctx.dev_alloc(m * 32) for _ in range(3)]
    d_z = ctx.dev_alloc(z.nbytes)
    try:
        ctx.upload(d_z, z)
        for p in d:
            ctx.upload(p, np.full(m * 4, 0xdeadbeefdeadbeef, np.uint64))
        if sliced is None:
            ctx.r1cs_eval_dev(dr, d_z, *d)
            return [ctx.download(p, rows * 32, np.uint64).reshape(-1, 4) for p in d]
        log_m, rank, log_w = sliced
        ctx.r1cs_eval_slice_dev(dr, d_z, log_m, rank, log_w, *d)
        return [ctx.download(p, (m >> log_w) * 32, np.uint64).reshape(-1, 4) for p in d]
    finally:
        for p in d + [d_z]:
            ctx.dev_free(p)


@pytest.fixture(scope='module')
def knobs(ctx):
    """minimum length and look-back in force, read off a system too small to have aliases"""
    cs, _, _ = ref.random_r1cs(1, 4, 2, 6)
    dr = ctx.load_r1cs(r1cs_product(fx.r1cs_to_csr(cs)))
    info = alias_info(dr)
    dr.free()
    assert info['aliases'] == 0 and info['min'] >= 1
    return info['min'], info['lookback']


# ---------------------------------------------------------------- 1. crafted system
@pytest.mark.parametrize('c_short', [False, True])
def test_crafted_repeats(ctx, oracle, knobs, c_short):
    min_len, back = knobs
    csr, mats, planted, never = crafted_system(min_len, back, c_short)
    assert (int(np.diff(mats[2][0].astype(np.int64)).max()) < BIN_MIN) == c_short
    rows = csr.num_gates + csr.num_input
    z = random_z(csr.num_input + csr.num_aux, 3)
    want = oracle.synthesize(csr, z)
    dr = ctx.load_r1cs(r1cs_product(csr))            # through the coefficient dictionary: equal values, equal indices
    try:
        info, table = alias_info(dr), alias_table(dr)
        expect, terms = reference_aliases(mats, min_len, back)
        assert table == expect and info['aliases'] == len(expect) and info['terms'] == terms
        assert set(planted) <= set(table), sorted(set(planted) - set(table))
        dsts, srcs = {(t[0], t[1]) for t in table}, {(t[2], t[3]) for t in table}
        assert len(dsts) == len(table) and not dsts & srcs                                # no alias of an alias
        assert not {(t[0], t[1]) for t in never} & dsts                                   # those rows are evaluated
        if c_short:
            assert all(t[0] != 2 for t in table) and any(t[2] == 2 for t in table)
        got = evaluate(ctx, dr, z, rows)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), 'matrix %d' % k
    finally:
        dr.free()


def test_nothing_binned_no_aliases(ctx, oracle, knobs, monkeypatch):
    """FK_SPMV_BIN_MIN=0: no class lists, hence no destinations -- zero aliases, same a, b, c"""
    csr, mats, planted, _ = crafted_system(*knobs, False)
    rows = csr.num_gates + csr.num_input
    z = random_z(csr.num_input + csr.num_aux, 4)
    want = oracle.synthesize(csr, z)
    monkeypatch.setenv('FK_SPMV_BIN_MIN', '0')
    dr = ctx.load_r1cs(r1cs_product(csr))
    try:
        assert alias_info(dr)['aliases'] == 0 and alias_table(dr) == []
        got = evaluate(ctx, dr, z, rows)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), 'matrix %d' % k
    finally:
        dr.free()


# ---------------------------------------------------------------- 2. - 4. the fixture transaction x 4, block-sorted with row windows
COPIES = 4


@pytest.fixture(scope='module')
def rollup4(oracle):
    """(num_input, num_aux, mats, table, R1csC, z, the oracle's a, b, c): computed once, never written to"""
    import bench
    n_in, n_aux, mats, table = bench.materialise_rollup(COPIES)
    csr = fx.co.R1csC(n_in, n_aux, *[fx.co.Csr(ptr, col, np.ascontiguousarray(table[cidx])) for ptr, col, cidx in mats])
    inst, zs = bench.load_rollup_instance()
    z = bench.tile_witness(zs[:3], inst.num_input, COPIES)
    return n_in, n_aux, mats, table, csr, z, oracle.synthesize(csr, z), inst


def test_fixture_system_aliases_and_outputs(ctx, knobs, rollup4):
    """77 080 gates, 3.77 M terms: block-sorted lists with row windows.  Under the defaults (minimum 4, look-back 8) the restated rule finds
    9 922 aliases per transaction standing for 278 613 terms (5 084 B = A in the same gate, 4 833 B = A two gates back, 5 one gate back
    inside A or B); without a look-back limit 9 924 for 279 122 terms."""
    n_in, n_aux, mats, table, csr, z, want, _ = rollup4
    assert csr.num_gates == 77080 and sum(int(m[0][-1]) for m in mats) == 4 * 941985
    dr = ctx.load_r1cs_coded(n_in, n_aux, mats, table)
    try:
        assert dr.windows() is not None
        expect, terms = reference_aliases(mats, *knobs)
        info, got_table = alias_info(dr), alias_table(dr)
        assert got_table == expect and info['terms'] == terms              # the restated rule is the authority
        if knobs == (4, 8):
            assert info["aliases"] == 4 * 9922
        got = evaluate(ctx, dr, z, csr.num_gates + n_in)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), 'matrix %d' % k
    finally:
        dr.free()


def _child(env, mode):
    e = {k: v for k, v in os.environ.items() if not k.startswith(('FK_SPMV_', 'FK_PROVE_'))}
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_dedup_child.py'), mode], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (env, out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines() if l.startswith('PROOFS ')]
    assert len(line) == 1, out.stdout[-1000:]
    return line[0].split()[1:]


def test_proof_bytes_with_and_without_dedup():
    """fk_prove_r1cs (chunked hand-over: the window path) and fk_prove_r1cs_submit / _wait give the same 256 bytes with FK_SPMV_DEDUP unset
    and = 0; the switch is read once, hence a fresh process per setting"""
    on, off = _child({}, 'plain'), _child({'FK_SPMV_DEDUP': '0'}, 'plain')
    assert int(on[0]) == 4 * 9922 and int(off[0]) == 0                    # aliases in force
    assert len(on[1]) == 512 and on[1] == on[2] == off[1] == off[2]


def replace_row(mat, g, col, cidx):
    ptr, c, i = mat
    lo, hi = int(ptr[g]), int(ptr[g + 1])
    ptr2 = ptr.astype(np.int64)
    ptr2[g + 1:] += len(col) - (hi - lo)
    return ptr2.astype(np.uint64), np.concatenate([c[:lo], col, c[hi:]]).astype(np.uint32), np.concatenate([i[:lo], cidx, i[hi:]]).astype(np.uint32)


def test_aliases_across_window_boundaries(ctx, oracle, knobs, rollup4):
    """an alias whose source is the last gate of window 0 and whose destination, two gates on, opens window 1; another with source and
    destination in the last block of window 1.  a, b, c against the oracle; the chunked proof (one evaluation per window) against the
    whole-witness one"""
    n_in, n_aux, mats, table, _, z, _, _ = rollup4
    dr0 = ctx.load_r1cs_coded(n_in, n_aux, mats, table)
    w = dr0.windows()
    dr0.free()
    assert w is not None and len(w['rows']) >= 4
    e0, e1 = w['rows'][1] - 1, w['rows'][2] - 1
    rng = np.random.default_rng(12)
    mats = list(mats)
    planted = []
    for src_g, dst_g in ((e0, e0 + 2), (e1 - 2, e1)):
        hi = int(max(mats[0][1][int(mats[0][0][src_g]):int(mats[0][0][src_g + 1])].max(initial=0), n_in + 100))      # variables the neighbourhood already reads
        col, cidx = rng.integers(hi - 90, hi, 21).astype(np.uint32), rng.integers(0, len(table), 21).astype(np.uint32)
        mats[0] = replace_row(mats[0], src_g, col, cidx)
        mats[1] = replace_row(mats[1], dst_g, col, cidx)
        planted.append((1, dst_g, 0, src_g))
    csr = fx.co.R1csC(n_in, n_aux, *[fx.co.Csr(ptr, col, np.ascontiguousarray(table[cidx])) for ptr, col, cidx in mats])
    want = oracle.synthesize(csr, z)
    dr = ctx.load_r1cs_coded(n_in, n_aux, mats, table)
    key = None
    d_z = ctx.dev_alloc(z.nbytes)
    try:
        w2 = dr.windows()
        assert w2 is not None and w2['rows'] == w['rows']
        got_table = alias_table(dr)
        assert got_table == reference_aliases(mats, *knobs)[0] and set(planted) <= set(got_table)
        got = evaluate(ctx, dr, z, csr.num_gates + n_in)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), 'matrix %d' % k
        key, _ = ctx.setup(r1cs_product(csr), **{k: fx.mont_fr(v) for k, v in TOXIC.items()})
        r, s = fx.mont_fr(0x1111), fx.mont_fr(0x2222)
        z2 = random_z(len(z), 9)
        ctx.upload(d_z, z2)
        other = ctx.prove_witness_dev(key, dr, d_z, r, s)         # leaves ANOTHER witness's a, b, c in the staging buffers
        chunked = ctx.prove_witness(key, dr, z, r, s)
        ctx.upload(d_z, z)
        whole = ctx.prove_witness_dev(key, dr, d_z, r, s)
        assert chunked.tobytes() == whole.tobytes() != other.tobytes()
    finally:
        ctx.dev_free(d_z)
        dr.free()
        if key is not None:
            key.free()


def test_tiled_and_sliced_evaluations_unchanged(ctx, rollup4):
    """where the dedup set does not apply -- a tiled load, a cyclic slice of the explicit system -- the full lists are evaluated as before"""
    n_in, n_aux, mats, table, csr, z, want, inst = rollup4
    rows = csr.num_gates + n_in
    log_m = max(rows - 1, 1).bit_length()
    dt = ctx.load_r1cs(inst, copies=COPIES)
    try:
        assert alias_info(dt)['aliases'] == 0
        got = evaluate(ctx, dt, z, rows)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), 'tiled, matrix %d' % k
    finally:
        dt.free()
    dr = ctx.load_r1cs_coded(n_in, n_aux, mats, table)
    try:
        assert alias_info(dr)['aliases'] > 0
        for log_w, rank in ((1, 1), (2, 2)):
            got = evaluate(ctx, dr, z, rows, sliced=(log_m, rank, log_w))
            for k in range(3):
                full = np.zeros((1 << log_m, 4), np.uint64)
                full[:rows] = want[k]
                assert np.array_equal(got[k], full[rank::1 << log_w]), (log_w, rank, k)
    finally:
        dr.free()
