"""The plan of a resident constraint system without a GPU (csrc/spmv_plan.hpp through fk_r1cs_plan_host, which runs the loader's own
stages): class lists, block ordering, launch segments, wave range, row windows, the alias plan and its dedup lists, the query lists, the
refusals.  Every expectation is restated here from the rule, with numpy; every comparison is exact.  The GPU tests compare a, b, c with the
oracle and would pass with a lost block order or class order -- these would not."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import fawkes_crypto_amd as fk
from helpers import r1cs_product
import spmv_plan_cases as pc

FK_ERR_BAD_ARG = 1
CLS_LO, CLS_LG, CAP = (64, 32, 16, 8, 0), (4, 3, 2, 1, 0), 1024        # length classes: lanes per row 16, 8, 4, 2, 1; the sort key is min(length, CAP)
BLOCK, WINDOWS = 4096, 8                                               # FK_SPMV_BLOCK_ROWS, FK_SPMV_WINDOWS (compiled-in defaults)
WAVE_LO, WAVE_HI = 4, 64


@pytest.fixture(scope='module', autouse=True)
def _oracle(oracle):
    return oracle


@pytest.fixture(scope='module')
def lib():
    return fk.api.load_library()


@pytest.fixture(scope='module')
def table():
    return np.stack([fx.mont_fr(v) for v in (1, 2, 3, 5, 7)])


def system(rng, lens, nv, n_table=5):
    """three (ptr, col, cidx) with the given row lengths per matrix, random columns and coefficient indices"""
    mats = []
    for ln in lens:
        ptr = np.zeros(len(ln) + 1, np.uint64)
        ptr[1:] = np.cumsum(ln)
        nnz = int(ptr[-1])
        mats.append((ptr, rng.integers(0, nv, nnz).astype(np.uint32), rng.integers(0, n_table, nnz).astype(np.uint32)))
    return mats


def class_of(ln):
    return np.searchsorted(-np.array(CLS_LO), -np.minimum(ln, CAP), side='left')       # first c with CLS_LO[c] <= length


def expected_list(ln, blocked):
    """class by class; inside a class longest first and stable -- over the whole system, or inside ascending blocks of BLOCK rows"""
    g = np.arange(len(ln))
    key = np.minimum(ln, CAP)
    block = g // BLOCK if blocked else np.zeros(len(ln), np.int64)
    return g[np.lexsort((g, -key, block, class_of(ln)))].astype(np.uint32)


def expected_segs(groups_per_class):
    """[(matrix, class, rows)] -> the segment table and the block count, by the recurrence first_block[s + 1] = first_block[s] + ceil(groups / (256 >> lg))"""
    out, first = [], 0
    for k, lg, rows, off, groups in groups_per_class:
        out.append((k, lg, rows, off, first))
        first += -(-groups // (256 >> lg))
    return out, first


def full_segs(lens, binned, copies):
    segs = []
    for k in range(3):
        if not binned[k]:
            continue
        cls, off = class_of(lens[k]), 0
        for c in range(5):
            n = int((cls == c).sum())
            if n:
                segs.append((k, CLS_LG[c], n, off, n * copies))
            off += n
    return expected_segs(segs)


def check_lists(plan, lens, copies, blocked):
    gates = len(lens[0])
    binned = [gates > 0 and int(ln.max(initial=0)) >= pc.BIN_MIN for ln in lens]
    assert plan['info'].segs.mask == sum(1 << k for k in range(3) if binned[k])
    for k in range(3):
        lst = plan['lists'][k]
        if not binned[k]:
            assert lst is None
            continue
        assert np.array_equal(np.sort(lst), np.arange(gates))                                  # every gate exactly once
        assert np.array_equal(lst, expected_list(lens[k], blocked)), 'matrix %d' % k
        w0, w1 = plan['info'].wave_from[k], plan['info'].wave_to[k]
        if not blocked:                                                                        # (the wave kernel takes rows of tiled systems: never block-sorted)
            assert set(lst[w0:w1].tolist()) == set(np.flatnonzero((lens[k] >= WAVE_LO) & (lens[k] < WAVE_HI)).tolist())
    assert plan['segs'] == full_segs(lens, binned, copies)
    for k, lg, rows, off, _ in plan['segs'][0]:                                                # class c holds exactly the rows of CLS_LO[c] <= length < CLS_LO[c - 1]
        c = CLS_LG.index(lg)
        ln = lens[k][plan['lists'][k][off:off + rows]]
        assert (ln >= CLS_LO[c]).all() and (c == 0 or (ln < CLS_LO[c - 1]).all())
        if not blocked:
            assert (np.diff(np.minimum(ln, CAP)) <= 0).all()                                   # longest first
    return binned


# ---------------------------------------------------------------- crafted system: the alias table
@pytest.mark.parametrize('c_short', [False, True])
def test_crafted_aliases(lib, table, c_short):
    knobs = pc.plan_host(lib, 2, 2, system(np.random.default_rng(0), [np.ones(4, np.int64)] * 3, 4), table)['info']
    min_len, back = int(knobs.alias_min), int(knobs.alias_lookback)
    assert knobs.n_alias == 0 and min_len >= 1
    csr, mats, planted, never = pc.crafted_system(min_len, back, c_short)
    product = r1cs_product(csr)                          # through the coefficient dictionary: equal values, equal indices
    plan = pc.plan_struct(lib, product.struct)
    expect, terms = pc.reference_aliases(mats, min_len, back)
    assert plan['aliases'] == expect and plan['info'].n_alias == len(expect) and plan['info'].alias_terms == terms
    assert set(planted) <= set(plan['aliases'])
    assert not {(t[0], t[1]) for t in never} & {(t[0], t[1]) for t in plan['aliases']}        # those rows are evaluated
    assert (plan['info'].segs.mask == 3) == c_short
    coded = pc.plan_host(lib, csr.num_input, csr.num_aux, mats, np.stack([fx.mont_fr(1)] * 43))      # the coded path sees the indices alone
    assert coded['aliases'] == expect


# ---------------------------------------------------------------- class lists, segments, wave range
@pytest.mark.parametrize('copies', [1, 64])
def test_class_lists_every_boundary(lib, table, copies):
    rng = np.random.default_rng(11)
    lens = [rng.choice([3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 1500], size=300) for _ in range(3)]
    plan = pc.plan_host(lib, 3, 50, system(rng, lens, 53), table, copies)
    assert check_lists(plan, lens, copies, False) == [True] * 3
    assert plan['info'].win_k == 0


@pytest.mark.parametrize('copies', [1, 64])
def test_short_matrix_is_not_binned(lib, table, copies):
    rng = np.random.default_rng(12)
    lens = [rng.choice([1, 2, 9, 40], size=300), rng.choice([0, 1, 7], size=300), rng.choice([1, 8], size=300)]
    lens[1][5] = 7
    plan = pc.plan_host(lib, 3, 50, system(rng, lens, 53), table, copies)
    assert check_lists(plan, lens, copies, False) == [True, False, True]


def test_no_gates(lib, table):
    empty = [np.zeros(0, np.int64)] * 3
    plan = pc.plan_host(lib, 2, 3, system(np.random.default_rng(1), empty, 5), table, 1)
    assert check_lists(plan, empty, 1, False) == [False] * 3 and plan['segs'] == ([], 0) and plan['aliases'] == []
    assert plan['idx_a'].tolist() == [0, 1] and plan['idx_b'].tolist() == []
    st, keep, cidx = pc.coded_struct(2, 3, system(np.random.default_rng(1), empty, 5))
    rc, err = pc.plan_host_raw(lib, st, 64, cidx, table.ctypes.data, len(table), pc.PlanInfo())       # 64 copies of no gates: refused, as the loader refuses it
    assert rc == FK_ERR_BAD_ARG and '64 copies of this system do not fit' in err


# ---------------------------------------------------------------- block ordering, row windows, dedup lists
def blocked_system(rng, gates, nv):
    """every matrix has rows in all classes; B repeats A's row in ~3 % of the gates (aliases in B), C repeats A's row of the gate before in ~1 %"""
    lens = [rng.choice([1, 1, 2, 3, 5, 9, 17, 33, 70], size=gates) for _ in range(3)]
    same_b = np.flatnonzero((rng.random(gates) < 0.03) & (lens[0] >= 4))
    same_c = np.flatnonzero((rng.random(gates) < 0.01) & (np.roll(lens[0], 1) >= 4))
    same_c = same_c[same_c > 0]
    lens[1][same_b] = lens[0][same_b]
    lens[2][same_c] = lens[0][same_c - 1]
    mats = system(rng, lens, nv)
    pa = mats[0][0].astype(np.int64)
    for k, rows, shift in ((1, same_b, 0), (2, same_c, 1)):
        pk = mats[k][0].astype(np.int64)
        for g in rows.tolist():
            for arr in (1, 2):
                mats[k][arr][pk[g]:pk[g + 1]] = mats[0][arr][pa[g - shift]:pa[g - shift + 1]]
    return lens, mats


def prefix_counts(lst, segs, win_row):
    """per window bound and segment: how many of the segment's entries lie below the bound; they must be a prefix of the segment"""
    out = np.zeros((len(win_row), pc.SEGS), np.uint32)
    for s, (k, _, rows, off, _) in enumerate(segs):
        seg = lst[k][off:off + rows]
        for j, bound in enumerate(win_row):
            n = int((seg < bound).sum())
            assert (seg[:n] < bound).all() and (seg[n:] >= bound).all(), (j, s)
            out[j, s] = n
    return out


@pytest.mark.parametrize('gates', [16 * BLOCK, 16 * BLOCK - 1])
def test_block_order_windows_and_dedup_lists(lib, table, gates):
    """16 x 4096 gates is the smallest system whose lists are block-sorted and which has row windows; one gate fewer has neither"""
    rng = np.random.default_rng(13)
    lens, mats = blocked_system(rng, gates, 5000)
    plan = pc.plan_host(lib, 3, 4997, mats, table)
    info = plan['info']
    blocked = gates >= 16 * BLOCK
    assert check_lists(plan, lens, 1, blocked) == [True] * 3
    expect, terms = pc.reference_aliases(mats, int(info.alias_min), int(info.alias_lookback))
    assert plan['aliases'] == expect and info.alias_terms == terms and len(expect) > 1000
    # the dedup lists: the class lists minus the alias rows, in the same order; a matrix without aliases keeps its class list
    is_alias = [np.zeros(gates, bool) for _ in range(3)]
    for dm, dr, _, _ in expect:
        is_alias[dm][dr] = True
    assert [bool(info.own_dd[k]) for k in range(3)] == [bool(a.any()) for a in is_alias] == [False, True, True]
    segs_dd, off_dd, dd_lists = [], [0, 0, 0], []
    for k in range(3):
        want = plan['lists'][k][~is_alias[k][plan['lists'][k]]]
        dd_lists.append(want if info.own_dd[k] else plan['lists'][k])
        if info.own_dd[k]:
            assert np.array_equal(plan['lists_dd'][k], want)
    for k, lg, rows, off, _ in plan['segs'][0]:
        kept = int((~is_alias[k][plan['lists'][k][off:off + rows]]).sum())
        if kept:
            segs_dd.append((k, lg, kept, off_dd[k] if info.own_dd[k] else off, kept))
        off_dd[k] += kept
    assert plan['segs_dd'] == expected_segs(segs_dd) and info.segs_dd.mask == 7
    if not blocked:
        assert info.win_k == 0
        return
    for k, _, rows, off, _ in plan['segs'][0]:                     # inside a class the blocks ascend, longest first inside a block
        seg = plan['lists'][k][off:off + rows].astype(np.int64)
        blk, ln = seg // BLOCK, np.minimum(lens[k][seg], CAP)
        assert (np.diff(blk) >= 0).all() and (np.diff(ln)[np.diff(blk) == 0] <= 0).all()
    assert info.win_k == WINDOWS
    win_row = [int(info.win_row[j]) for j in range(WINDOWS + 1)]
    assert win_row == [gates if j == WINDOWS else gates * j // WINDOWS // BLOCK * BLOCK for j in range(WINDOWS + 1)]
    assert all(r % BLOCK == 0 for r in win_row[:-1]) and win_row[-1] == gates
    assert np.array_equal(plan['win_cnt'][:WINDOWS + 1], prefix_counts(plan['lists'], plan['segs'][0], win_row))
    assert np.array_equal(plan['win_cnt_dd'][:WINDOWS + 1], prefix_counts(dd_lists, plan['segs_dd'][0], win_row))
    dst_rows = np.array([t[1] for t in expect])
    assert [int(info.win_alias[j]) for j in range(WINDOWS + 1)] == [int((dst_rows < b).sum()) for b in win_row]


# ---------------------------------------------------------------- the threaded paths
def test_threaded_lists_and_alias_scan(lib, table, monkeypatch):
    """2^20 gates: the three lists are built side by side and the alias scan runs over 16 blocks of gates.  Every row is shorter than the
    minimum alias length except the planted ones, which sit at the 15 block boundaries ng * t / 16: a repeat 1 gate apart and one `lookback`
    gates apart that straddle the boundary (the scan of a block reads `lookback` gates into the block before it), and one lookback + 1 apart
    that must not be found.  The rule is restated (reference_aliases) over the gates within lookback + 4 of each boundary and over a seeded
    sample of cuts elsewhere; everywhere else no row reaches the minimum length, so the table must be exactly what the cuts give."""
    monkeypatch.setenv('FK_HOST_THREADS', '16')
    ng, nv = 1 << 20, 100000
    rng = np.random.default_rng(14)
    probe = pc.plan_host(lib, 2, 2, system(rng, [np.ones(4, np.int64)] * 3, 4), table)['info']
    min_len, back = int(probe.alias_min), int(probe.alias_lookback)
    assert 2 <= min_len <= 12 and back >= 1
    lens = [rng.integers(0, min_len, ng) for _ in range(3)]
    bounds = [ng * t // 16 for t in range(1, 16)]
    A, B, Cm = 0, 1, 2
    plants = []                                   # (src matrix, src gate, dst matrix, dst gate)
    for b in bounds:
        plants += [(A, b - 1, A, b), (B, b - 1, B, b - 1 + back), (Cm, b - 1, A, b + back)]
    assert len({(m, g) for p in plants for m, g in (p[:2], p[2:])}) == 2 * len(plants)
    for sm, sg, dm, dg in plants:
        lens[sm][sg] = lens[dm][dg] = 12
    mats = system(rng, lens, nv)
    ptrs = [m[0].astype(np.int64) for m in mats]
    for sm, sg, dm, dg in plants:
        for arr in (1, 2):
            mats[dm][arr][ptrs[dm][dg]:ptrs[dm][dg] + 12] = mats[sm][arr][ptrs[sm][sg]:ptrs[sm][sg] + 12]
    plan = pc.plan_host(lib, 3, nv - 3, mats, table)
    assert plan['info'].segs.mask == 7
    check_lists(plan, lens, 1, True)

    def cut(g0, g1):
        sub = [(m[0][g0:g1 + 1] - m[0][g0], m[1][int(m[0][g0]):int(m[0][g1])], m[2][int(m[0][g0]):int(m[0][g1])]) for m in mats]
        return [(dm, dr + g0, sm, sr + g0) for dm, dr, sm, sr in pc.reference_aliases(sub, min_len, back, binned=[True] * 3)[0]]

    expect = []
    for b in bounds:
        expect += cut(b - back - 4, b + back + 4)
    for g0 in rng.integers(0, ng - 2000, 8).tolist():
        assert cut(g0, g0 + 2000) == [t for t in expect if g0 <= t[1] < g0 + 2000]
    assert plan['aliases'] == expect == sorted([(A, b, A, b - 1) for b in bounds] + [(B, b - 1 + back, B, b - 1) for b in bounds], key=lambda t: (t[1], t[0]))


# ---------------------------------------------------------------- the query lists
@pytest.mark.parametrize('copies', [1, 3])
def test_query_lists_in_bellmans_order(lib, table, copies):
    rng = np.random.default_rng(15)
    nin, naux = 5, 40
    lens = [rng.choice([0, 1, 2, 9], size=60) for _ in range(3)]
    mats = system(rng, lens, nin + naux)
    mats[1][1][mats[1][1] == 2] = 3                                     # input 2 is in no B row
    plan = pc.plan_host(lib, nin, naux, mats, table, copies)
    a_aux = np.isin(np.arange(nin, nin + naux), mats[0][1])
    b_in, b_aux = np.isin(np.arange(nin), mats[1][1]), np.isin(np.arange(nin, nin + naux), mats[1][1])
    assert not b_in[2]
    # the tiled system's variables: ONE, every copy's inputs, every copy's aux variables; each copy repeats the instance's pattern
    t_in = 1 + copies * (nin - 1)
    b_in_all = np.concatenate([b_in[:1]] + [b_in[1:]] * copies)
    a_aux_all, b_aux_all = np.tile(a_aux, copies), np.tile(b_aux, copies)
    assert plan['idx_a'].tolist() == list(range(t_in)) + (t_in + np.flatnonzero(a_aux_all)).tolist()
    assert plan['idx_b'].tolist() == np.flatnonzero(b_in_all).tolist() + (t_in + np.flatnonzero(b_aux_all)).tolist()


# ---------------------------------------------------------------- refusals
def test_refusals(lib, table):
    rng = np.random.default_rng(16)
    lens = [np.full(6, 2)] * 3

    def call(mats=None, copies=1, tab=table, nin=2, naux=3, st=None, info=True):
        st_, keep, cidx = pc.coded_struct(nin, naux, mats if mats is not None else system(rng, lens, 5))
        return pc.plan_host_raw(lib, st_ if st is None else st, copies, cidx, tab.ctypes.data, len(tab), pc.PlanInfo() if info else None)

    assert call()[0] == 0
    assert pc.plan_host_raw(lib, None, 1, info=pc.PlanInfo())[0] == FK_ERR_BAD_ARG                # null arguments
    assert call(info=False)[0] == FK_ERR_BAD_ARG
    st, keep, _ = pc.coded_struct(2, 3, system(rng, lens, 5))
    st.b_ptr = None
    assert call(st=st) == (FK_ERR_BAD_ARG, 'r1cs: null row pointer')
    mats = system(rng, lens, 5)
    mats[2][0][3] = 1                                                                               # 0 2 4 1 8 ...
    assert call(mats=mats) == (FK_ERR_BAD_ARG, 'r1cs: row_ptr not monotone')
    mats = system(rng, lens, 5)
    mats[0][1][7] = 5
    assert call(mats=mats) == (FK_ERR_BAD_ARG, 'r1cs: variable index 5 out of range')
    assert call(copies=0) == (FK_ERR_BAD_ARG, 'r1cs: copies must be at least 1')
    assert call(tab=np.stack([fx.mont_fr(2), fx.mont_fr(1)])) == (FK_ERR_BAD_ARG, 'r1cs: coefficient table must start with ONE')
    mats = system(rng, lens, 5)
    mats[1][2][0] = 4
    assert call(mats=mats, tab=table[:3].copy()) == (FK_ERR_BAD_ARG, 'r1cs: coefficient index out of range')


# ---------------------------------------------------------------- the struct mirrors against the header
def test_plan_structs_mirror_the_header(tmp_path):
    """spmv_plan_cases.PlanSegs / PlanInfo are hand-written mirrors of fk_r1cs_plan_segs / fk_r1cs_plan_info: a C program over
    include/fawkes_hip_inspect.h prints the size of each struct and the offset of every field the mirrors name, and they must agree"""
    import os
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mirrors = (('fk_r1cs_plan_segs', pc.PlanSegs), ('fk_r1cs_plan_info', pc.PlanInfo))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fawkes_hip_inspect.h"', 'int main(void) {']
    for cname, mirror in mirrors:
        lines.append('    printf("%%zu", sizeof(%s));' % cname)
        lines += ['    printf(" %%zu", offsetof(%s, %s));' % (cname, f[0]) for f in mirror._fields_]
        lines.append('    printf("\\n");')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    out = subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for (cname, mirror), line in zip(mirrors, got):
        assert [int(x) for x in line.split()] == [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_], cname
