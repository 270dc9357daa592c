"""The back of a multiplication, stage by stage (csrc/msm.hip: msm_accumulate_kernel, msm_accumulate_merged_kernel, msm_overflow_kernel,
msm_overflow_fold_kernel, msm_bucket_reduce_kernel, msm_fold_partials_kernel, msm_level_kernel, the host's Horner in msm_end), run through
the product's own host code by fk_msm_back_dump and compared EXACTLY, on group elements, with the references of tests/_msm_back_ref.py:
each stage against the reference applied to what the device left one stage earlier, and against the chain from the bases.

The whole-multiplication tests (test_gpu_msm.py, test_gpu_precompute.py) see one group element at the very end.  These kernels are index
logic -- min(totals, cap), lo = cap + seg * SEG, the (window, position) cursor of the merged walk, lev + (w - 1) * n, grid-stride loops
over device-side counts, k = t * L, a 4-slot LDS fold -- and the shapes below are the ones at which that logic takes another turn.
Entries are placed with small scalars: d << offset_w puts a base into bucket d - 1 of window w and nowhere else.  cap, SEG_MIN, L, T,
nblk and B come from fk_msm_plan; every case asserts from the dump's dyn, tasks and obs that the path it names was taken."""
import ctypes as C

import numpy as np
import pytest

from _msm_back_ref import Back, BackOut, Group, entry, run_dump
from helpers import R
from test_gpu_msm import _digit_edge_scalars
from test_gpu_msm_front import windows

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ inputs
def gen_bases(ctx, g2, n, seed):
    """n distinct points made on the device (fk_gen_points_g1_dev / _g2_dev), as host rows"""
    pb = 128 if g2 else 64
    d = ctx.dev_alloc(n * pb)
    try:
        (ctx.gen_points_g2_dev if g2 else ctx.gen_points_g1_dev)(d, n, seed)
        return ctx.download(d, n * pb).reshape(n, pb).copy()
    finally:
        ctx.dev_free(d)


def plan(n, wb, merged=False):
    from fawkes_crypto_amd import api
    return api.msm_plan(n, wb, merged)


def check(ctx, g2, bases, ints, wb, merged, what):
    assert max(ints, default=0) < R
    return Back(run_dump(ctx, g2, bases, ints, wb, merged), what).check()


def solve_n(wb, size_of, guess):
    """the n with n == size_of(plan(n)): the plan's cap depends on n, the bucket sizes the case wants depend on the cap"""
    n = guess
    for _ in range(8):
        m = size_of(plan(n, wb))
        if m == n:
            return n
        n = m
    raise AssertionError('no fixed point for n')


# ------------------------------------------------------------------------------------------ accumulate edges
def edge_scalars(p, sizes, n):
    """window 0: digit k + 1 repeated sizes[k] times, then the special buckets; the rest of the n entries go one by one into other windows.
    Returns (scalars, {name: (first index, count)})"""
    win = windows(p)
    o0, cw0 = win[0]
    ints, at = [], {}

    def put(name, vals):
        at[name] = (len(ints), len(vals))
        ints.extend(vals)
    for k, s in enumerate(sizes):
        put(('size', k), [(k + 1) << o0] * s)
    d = len(sizes) + 1                   # digit d: nothing (bucket d - 1 stays empty)
    at['empty'] = d - 1
    put('cancel', [(d + 1) << o0, ((1 << cw0) - (d + 1)) << o0])          # +(d + 1) and, for the same base, raw 2^cw - (d + 1): the digit -(d + 1), a carry into window 1
    put('repeat', [(d + 2) << o0] * 6)                                   # one base six times: the second addition is a doubling
    put('inf', [(d + 3) << o0] * 5)                                      # two of its five bases at infinity
    rng = np.random.default_rng(len(sizes) * 7919 + n)
    fill = []
    while len(ints) + len(fill) < n:
        w = int(rng.integers(2, len(win)))
        o, cw = win[w]
        v = int(rng.integers(1, (1 << (cw - 1)) + 1)) << o
        if v < R:
            fill.append(v)
    put('fill', fill)
    assert len(ints) == n
    return ints, at


@pytest.mark.parametrize('g2', [False, True], ids=['g1', 'g2'])
def test_accumulate_edges(ctx, oracle, g2):
    """buckets of cap - 1, cap, cap + 1 (one task, 63 idle lanes), cap + SEG (exactly one full segment), cap + SEG + 1 (a second task of one
    entry) and cap + 2 SEG entries; an empty bucket; P and -P in one bucket; one base repeated (doubling); infinity bases inside a run and
    inside an oversized run.  G2: the same at half the size with two oversized buckets."""
    n, wb = (1500, 8) if g2 else (3000, 8)
    p = plan(n, wb)
    cap, seg = p['cap'], p['seg_min']
    assert (p['W'], p['B'], p['L']) == (32, 128, 1)
    sizes = [cap - 1, cap, cap + 1, cap + seg + 1] if g2 else [cap - 1, cap, cap + 1, cap + seg, cap + seg + 1, cap + 2 * seg]
    ints, at = edge_scalars(p, sizes, n)
    bases = gen_bases(ctx, g2, n, 31)
    i, _ = at['cancel']
    bases[i + 1] = bases[i]
    i, m = at['repeat']
    bases[i:i + m] = bases[i]
    i, _ = at['inf']
    bases[[i + 1, i + 3]] = 0
    i, m = at[('size', len(sizes) - 1)]                  # the largest oversized run: infinity below the cap, in the middle and at its very end
    bases[[i, i + 1, i + cap + 3, i + m - 1]] = 0
    b = check(ctx, g2, bases, ints, wb, False, ('accumulate edges', 'g2' if g2 else 'g1'))
    d, dyn = b.d, b.dyn
    assert dyn['cap'] == cap and dyn['seg'] == seg, dyn
    assert d['totals'][0, :len(sizes)].tolist() == sizes and d['totals'][0, at['empty']] == 0
    over = [k for k, s in enumerate(sizes) if s > cap]
    want_tasks = sorted((k, t) for k in over for t in range((sizes[k] - cap + seg - 1) // seg))
    assert sorted(map(tuple, d['tasks'].tolist())) == want_tasks and dyn['n_over'] == dyn['n_obs'] == len(over), (dyn, d['tasks'])
    assert [t for k, t in want_tasks].count(1) == (1 if g2 else 2)          # second tasks: of cap + SEG + 1 (one entry) and of cap + 2 SEG
    e = at['empty'] + 1                                                     # the cancel bucket follows the empty one
    assert d['totals'][0, e] == 2 and not d['buckets'][e].any(), 'accumulate: P + (-P) is not infinity'
    assert d['totals'][0, e + 1] == 6 and d['totals'][0, e + 2] == 5


# ------------------------------------------------------------------------------------------ overflow grids
@pytest.fixture(scope='module')
def grid_inputs(ctx):
    """90 digit values repeated in every window, each scalar cap + SEG + 1 times: 90 oversized buckets of two tasks in each of 22 windows"""
    wb = 12
    n = solve_n(wb, lambda p: 90 * (p['cap'] + p['seg_min'] + 1), 30000)
    p = plan(n, wb)
    assert (p['W'], p['B']) == (22, 2048)
    win = windows(p)
    digits = [7 * k + 3 for k in range(90)]              # at most 626: a top window's digit below r >> 244
    vals = [sum(dg << o for o, _ in win) for dg in digits]
    ints = [v for v in vals for _ in range(p['cap'] + p['seg_min'] + 1)]
    np.random.default_rng(12).shuffle(ints)
    assert len(ints) == n and max(ints) < R
    return wb, n, p, ints, gen_bases(ctx, False, n, 32)


@pytest.mark.parametrize('merged', [False, True], ids=['ordinary', 'merged'])
def test_overflow_grids_loop(ctx, oracle, grid_inputs, merged):
    """more tasks than msm_overflow_kernel's 2048 workgroups and more fold groups than msm_overflow_fold_kernel's 256: both grid-stride
    loops run a second time.  Merged: the 22 (window, bucket) pairs of one bucket share ONE fold group and each window reads its own level."""
    wb, n, p, ints, bases = grid_inputs
    b = check(ctx, False, bases, ints, wb, merged, ('overflow grids', 'merged' if merged else 'ordinary'))
    dyn = b.dyn
    many = min(max(2048, p['W'] * p['B'] // 8192), p['over_max'] - 64)
    assert dyn['n_over'] == 90 * p['W'] <= many and dyn['cap'] == p['cap'] and dyn['seg'] == p['seg_min'], dyn
    assert dyn['n_tasks'] == 2 * dyn['n_over'] > 2048, dyn
    if merged:
        assert dyn['n_obs'] == 90 and (b.d['obs'][:, 2] == 2 * p['W']).all(), dyn
        assert len(set((b.d['tasks'][:, 0] // p['B']).tolist())) == p['W']          # tasks of every window, i.e. of every level
    else:
        assert dyn['n_obs'] == dyn['n_over'] > 256, dyn


def test_one_long_fold_group(ctx, oracle):
    """one bucket of cap + 257 SEG_MIN + 1 entries: its fold group has more tasks than the fold workgroup has lanes (the k += 256 loop)"""
    wb = 8
    n = solve_n(wb, lambda p: p['cap'] + 257 * p['seg_min'] + 1, 67000)
    p = plan(n, wb)
    ints = [5 << windows(p)[0][0]] * n
    b = check(ctx, False, gen_bases(ctx, False, n, 33), ints, wb, False, 'one long fold group')
    assert b.dyn['seg'] == p['seg_min'] and b.dyn['n_obs'] == 1 and b.d['obs'][0].tolist() == [4, 0, 258], (b.dyn, b.d['obs'])
    assert b.d['obs'][0, 2] > 256


# ------------------------------------------------------------------------------------------ bucket reduction
def reduce_scalars(p, n):
    """the digit-edge scalars of test_gpu_msm.py and entries placed at the reduction's corners, in a wide and in a narrow window: buckets 0,
    L - 1, L (a lane's last and the next lane's first), 255 L, 256 L (the last lane of a block, the first of the next), the last lane's first
    and last bucket and the window's top bucket (digit 2^(cw-1), which stays positive)"""
    win = windows(p)
    L, T = p['L'], p['T']
    placed = []
    for w in sorted({0, min(p['wide'], p['W'] - 1), p['W'] - 1}):
        o, cw = win[w]
        top = 1 << (cw - 1)
        for bkt in (0, L - 1, L, 255 * L, 256 * L, (T - 1) * L, (top // L - 1) * L, top - 1, p['B'] - 1):
            if bkt < top and ((bkt + 1) << o) < R:
                placed.append((w, bkt, (bkt + 1) << o))
    edge = _digit_edge_scalars(p['c'])
    ints = [v for _, _, v in placed]
    assert len(ints) <= n
    ints += (edge * (n // len(edge) + 1))[:n - len(ints)]
    return ints, placed


REDUCE_L = {8: 1, 14: 2, 16: 8, 17: 16, 19: 64, 22: 64}


@pytest.mark.parametrize('g2,wb,merged', [(False, c, False) for c in REDUCE_L] + [(False, 16, True), (False, 19, True), (True, 14, False)],
                         ids=['g1-c%d' % c for c in REDUCE_L] + ['g1-c16-merged', 'g1-c19-merged', 'g2-c14'])
def test_bucket_reduction_corners(ctx, oracle, g2, wb, merged):
    n = 300
    p = plan(n, wb, merged)
    assert p['c'] == wb and p['L'] == (min(REDUCE_L[wb], 8) if merged else REDUCE_L[wb]) and p['T'] * p['L'] == p['B']
    ints, placed = reduce_scalars(p, n)
    b = check(ctx, g2, gen_bases(ctx, g2, n, 34 + wb), ints, wb, merged, ('reduction', g2, wb, merged))
    for w, bkt, _ in placed:
        assert b.d['totals'][w, bkt] >= 1, ('reduction: no entry reached its bucket', w, bkt)
    assert any(bkt == p['B'] - 1 for _, bkt, _ in placed) and any(bkt == 256 * p['L'] for _, bkt, _ in placed) == (p['B'] > 256 * p['L'])
    assert b.have_buckets == (wb < 19 or merged)          # c >= 19, ordinary form: checked from winparts onward
    assert p['nblk'] == (p['T'] + 255) // 256 and (p['nblk'] > 1) == (wb >= 14)


# ------------------------------------------------------------------------------------------ levels
def level_variants(n, nb):
    """sets of positions at infinity: none; 0; 1; n - 1; one whole group of NB points"""
    out = []
    for v in ((), (0,), (1,), (n - 1,), tuple(range(nb))):
        v = tuple(i for i in v if i < n)
        if v not in out:
            out.append(v)
    return out


@pytest.mark.parametrize('g2,n', [(False, n) for n in (1, 2, 3, 5, 1027)] + [(True, n) for n in (1, 2, 3, 1025)],
                         ids=['g1-n%d' % n for n in (1, 2, 3, 5, 1027)] + ['g2-n%d' % n for n in (1, 2, 3, 1025)])
@pytest.mark.parametrize('wb', [8, 16])
def test_levels(ctx, oracle, g2, n, wb):
    """msm_level_kernel with n not a multiple of the NB points that share an inversion (4 in G1, 2 in G2), more than one workgroup, and
    points at infinity inside a batch -- first, second, last, and a whole batch: a merged multiplication whose every stage is checked"""
    nb = 2 if g2 else 4
    rng = np.random.default_rng(n * 100 + wb + g2)
    clean = gen_bases(ctx, g2, n, 35)
    ints = [int.from_bytes(rng.bytes(40), 'little') % R for _ in range(n)]
    variants = level_variants(n, nb) if n < 64 else [(0, 1, n - 1) + tuple(range(2 * nb, 3 * nb))]
    for inf in variants:
        bases = clean.copy()
        bases[list(inf)] = 0
        b = check(ctx, g2, bases, ints, wb, True, ('levels', g2, n, wb, inf))
        lev = b.d['levels']
        assert lev.shape[0] == b.W - 1 and all(not lev[:, i].any() for i in inf)
        assert all(lev[:, i].any(axis=1).all() for i in range(n) if i not in inf)


# ------------------------------------------------------------------------------------------ guards
def test_dump_of_nothing_writes_nothing(ctx):
    out = BackOut()
    guard = np.full(64, 0xa5, np.uint8)
    for f, _ in BackOut._fields_:
        if not f.endswith('_cap'):
            setattr(out, f, guard.ctypes.data)
    out.tasks_cap = out.obs_cap = out.buckets_cap = out.partials_cap = 1
    d = ctx.dev_alloc(64)
    try:
        for g2 in (0, 1):
            for merged in (0, 1):
                ctx.msm_back_dump(entry(ctx.lib), out, d, d, 0, g2=g2, merged=merged)
    finally:
        ctx.dev_free(d)
    assert (guard == 0xa5).all()


def test_dump_is_refused_while_a_proof_holds_the_lanes(ctx, oracle):
    """... and a whole multiplication after a dump still matches the oracle: the lane state is left sound"""
    import fawkes_crypto_amd as fk
    m, v_in = 1 << 10, 4
    v_aux = m - v_in
    key = ctx.synthetic_key(m, v_in, v_aux, m, m, seed=7)
    bufs = [ctx.dev_alloc(m * 32), ctx.dev_alloc(m * 32), ctx.dev_alloc(v_aux), ctx.dev_alloc(v_in), ctx.dev_alloc(v_aux)]
    d_z, d_h, d_da, d_dbi, d_dba = bufs
    n = 40
    bases = gen_bases(ctx, False, n, 36)
    ints = list(range(1, n + 1))
    try:
        ctx.upload(d_da, np.ones(v_aux, np.uint8)); ctx.upload(d_dbi, np.ones(v_in, np.uint8)); ctx.upload(d_dba, np.ones(v_aux, np.uint8))
        ctx.gen_scalars_dev(d_z, m, 9, 1)
        ctx.gen_scalars_dev(d_h, m, 10, 0)
        ctx.prove_msms_z_begin_dev(key, d_z, d_da, d_dbi, d_dba)
        try:
            with pytest.raises(fk.FkError) as e:
                run_dump(ctx, False, bases, ints, 0, False)
            assert e.value.code == 1 and 'a proof is in flight' in str(e.value)
        finally:
            ctx.prove_msms_finish_dev(key, d_h)
    finally:
        for p in bufs:
            ctx.dev_free(p)
        key.free()
    G = Group(False)
    for merged in (False, True):
        b = check(ctx, False, bases, ints, 0, merged, ('after the refusal', merged))
        big = gen_bases(ctx, False, 500, 37)
        sc = b.d['scalars'][np.arange(500) % n]
        assert ctx.msm_g1(big, sc).tobytes() == oracle.msm_g1(big, sc).tobytes(), 'a multiplication after a dump differs from the oracle'
    assert G.inf == bytes(64)
