"""Shared by tests/test_gpu_spmv_dedup.py and tests/test_r1cs_plan_host.py: the alias rule restated (`reference_aliases`), the crafted system
with every case of it planted, and fk_r1cs_plan_host (include/fawkes_hip_inspect.h: test-only, so its ctypes prototype is declared here,
like the other inspection entries' in the tests that call them)."""
import ctypes as C

import numpy as np

import bn254_ref as ref
import fixtures as fx

BIN_MIN = 8          # a matrix with a row this long has the length-class lists (spmv_plan.hpp: bin_min)
SEGS, WIN_MAX = 15, 16


def reference_aliases(mats, min_len, lookback, bin_min=BIN_MIN, binned=None):
    """The rule, restated: gates in row order, matrices A, B, C inside a gate.  A row of >= min_len terms of a binned matrix is an alias of
    the EARLIEST row, of any matrix, at most `lookback` gates back (its own gate included, matrices before it) whose column sequence and
    coefficient-index sequence are identical and which is not an alias itself.  mats: three (ptr, col, cidx).  binned: which matrices have
    class lists, where `mats` is a cut of a larger system and cannot tell.  Returns
    ([(dst matrix, dst row, src matrix, src row)] in (dst row, dst matrix) order, terms the aliases stand for)."""
    gates = len(mats[0][0]) - 1
    ptrs = [np.asarray(m[0]).astype(np.int64) for m in mats]
    if binned is None:
        binned = [gates > 0 and int(np.diff(p).max(initial=0)) >= bin_min for p in ptrs]
    window, out, terms = [], [], 0            # window: per gate, [(matrix, content, is alias)]
    for g in range(gates):
        cur = []
        window.append((g, cur))
        if len(window) > lookback + 1:
            window.pop(0)
        for k in range(3):
            lo, hi = int(ptrs[k][g]), int(ptrs[k][g + 1])
            if hi - lo < min_len:
                continue
            content = (mats[k][1][lo:hi].tobytes(), mats[k][2][lo:hi].tobytes())
            src = None
            if binned[k]:
                src = next(((k2, g2) for g2, rows in window for k2, c2, al2 in rows if not al2 and c2 == content), None)
            if src is not None:
                out.append((k, g, src[0], src[1]))
                terms += hi - lo
            cur.append((k, content, src is not None))
    return out, terms


def crafted_system(min_len, back, c_short, seed=7):
    """~3000 gates of random short and middling rows with every case planted 40 gates apart.  c_short: C's rows stay below BIN_MIN terms,
    so C has no class lists -- its rows can be sources and never destinations.  Returns (R1csC, [(ptr, col, cidx)] * 3, expected aliases,
    rows that must not be aliases)."""
    rng = np.random.default_rng(seed)
    gates, nin, naux = 3000, 3, 3100
    nv = nin + naux
    coeffs = fx.co.limbs_arr([1, ref.R - 1, 2] + [int(x) for x in rng.integers(3, 2**62, 40)])
    coeffs = np.stack([fx.mont_fr(int.from_bytes(c.tobytes(), 'little')) for c in coeffs])

    def row(n):
        return rng.integers(0, nv, n).astype(np.uint32), rng.integers(0, len(coeffs), n).astype(np.uint32)

    fill = [[0, 1, 1, 2, 3, 5, 9, 20], [0, 1, 1, 2, 3, 4, 8, 33], [0, 1, 2, 3] if c_short else [0, 1, 2, 3, 5, 12, 40]]
    rows = [[row(int(n)) for n in rng.choice(fill[k], size=gates)] for k in range(3)]
    A, B, Cm = 0, 1, 2
    want, never = [], []
    p = [20]

    def site():
        p[0] += 40
        assert back < 18 and p[0] + 2 * back + 2 < gates
        return p[0] - 40

    for n in (3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 512):          # every class boundary; A row g = B row g
        g = site()
        rows[A][g] = rows[B][g] = row(n)
        (want if n >= min_len else never).append((B, g, A, g))
    g = site(); rows[A][g] = rows[B][g + 2] = row(20); want.append((B, g + 2, A, g))                      # A row g = B row g + 2
    g = site(); rows[A][g] = rows[B][g + 1] = rows[A][g + 2] = row(17)                                      # three times
    want += [(B, g + 1, A, g), (A, g + 2, A, g)]
    g = site(); rows[A][g] = rows[B][g] = rows[A][g + back // 2] = rows[B][g + back] = row(33)              # four times: all point at the first
    want += [(B, g, A, g), (A, g + back // 2, A, g), (B, g + back, A, g)]
    g = site(); rows[Cm][g] = rows[A][g + 1] = row(5 if c_short else 16); want.append((A, g + 1, Cm, g))   # source in C, destination in A
    g = site(); c, i = row(24); i2 = i.copy(); i2[11] = (i2[11] + 1) % len(coeffs)                         # one coefficient index differs
    rows[A][g], rows[B][g] = (c, i), (c, i2); never.append((B, g, A, g))
    g = site(); c, i = row(24); perm = np.roll(np.arange(24), 1)                                            # same terms, another order
    rows[A][g], rows[B][g] = (c, i), (c[perm], i[perm]); never.append((B, g, A, g))
    g = site(); rows[A][g] = rows[A][g + back] = row(12); want.append((A, g + back, A, g))                  # exactly `back` gates apart
    g = site(); rows[A][g] = rows[A][g + back + 1] = row(12); never.append((A, g + back + 1, A, g))        # one gate further
    g = site(); rows[B][g] = rows[B][g + back] = rows[B][g + 2 * back] = row(9)                             # the middle one is an alias: no source for the third
    want.append((B, g + back, B, g)); never.append((B, g + 2 * back, B, g + back)); never.append((B, g + 2 * back, B, g))
    if c_short:                                                                                             # an unbinned matrix's repeat is never a destination
        g = site(); rows[A][g] = rows[Cm][g] = row(6); never.append((Cm, g, A, g))

    mats, csrs = [], []
    for k in range(3):
        ptr = np.zeros(gates + 1, np.uint64)
        ptr[1:] = np.cumsum([len(r[0]) for r in rows[k]])
        col = np.concatenate([r[0] for r in rows[k]]).astype(np.uint32)
        cidx = np.concatenate([r[1] for r in rows[k]]).astype(np.uint32)
        mats.append((ptr, col, cidx))
        csrs.append(fx.co.Csr(ptr, col, np.ascontiguousarray(coeffs[cidx])))
    return fx.co.R1csC(nin, naux, *csrs), mats, want, never


# ---------------------------------------------------------------- fk_r1cs_plan_host
class PlanSegs(C.Structure):
    """fk_r1cs_plan_segs"""
    _fields_ = [('nseg', C.c_uint32), ('mask', C.c_uint32)] + [(f, C.c_uint32 * SEGS) for f in ('mtx', 'lg', 'rows', 'list_off')] + [('first_block', C.c_uint32 * (SEGS + 1))]

    def table(self):
        """[(matrix, lg, rows, list offset, first block)] and the launch's block count"""
        return [(self.mtx[s], self.lg[s], self.rows[s], self.list_off[s], self.first_block[s]) for s in range(self.nseg)], self.first_block[self.nseg]


class PlanInfo(C.Structure):
    """fk_r1cs_plan_info"""
    _fields_ = [('list', C.c_void_p * 3), ('list_dd', C.c_void_p * 3)] + [(f, C.c_void_p) for f in (
        'alias_dst_mtx', 'alias_dst_row', 'alias_src_mtx', 'alias_src_row', 'idx_a', 'idx_b')] + [
        ('segs', PlanSegs), ('segs_dd', PlanSegs), ('own_dd', C.c_uint32 * 3), ('n_dd', C.c_uint32 * 3), ('wave_from', C.c_uint32 * 3), ('wave_to', C.c_uint32 * 3),
        ('win_k', C.c_uint32), ('win_row', C.c_uint64 * (WIN_MAX + 1)), ('win_alias', C.c_uint64 * (WIN_MAX + 1)),
        ('win_cnt', C.c_uint32 * SEGS * (WIN_MAX + 1)), ('win_cnt_dd', C.c_uint32 * SEGS * (WIN_MAX + 1))] + [(f, C.c_uint64) for f in (
        'n_alias', 'alias_terms', 'alias_min', 'alias_lookback', 'n_idx_a', 'n_idx_b')]


def plan_host_raw(lib, cs_struct, copies, cidx=(None, None, None), table=None, n_table=0, info=None):
    """the bare call: (code, fk_last_error(NULL))"""
    fn = lib.fk_r1cs_plan_host
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    rc = fn(C.byref(cs_struct) if cs_struct is not None else None, copies, *cidx, table, n_table, C.byref(info) if info is not None else None)
    return rc, (lib.fk_last_error(None) or b'').decode()


def coded_struct(num_input, num_aux, mats):
    """(fk_r1cs over the coded system's arrays, the arrays it points into, the three cidx pointers)"""
    from fawkes_crypto_amd._abi import R1csStruct
    st = R1csStruct()
    st.num_input, st.num_aux, st.num_gates = num_input, num_aux, len(mats[0][0]) - 1
    keep = []
    for nm, (ptr, col, ci) in zip('abc', mats):
        ptr = np.ascontiguousarray(ptr, np.uint64); col = np.ascontiguousarray(col, np.uint32); ci = np.ascontiguousarray(ci, np.uint32)
        assert len(col) == len(ci) == int(ptr[-1])
        keep.append((ptr, col, ci))
        setattr(st, nm + '_ptr', ptr.ctypes.data); setattr(st, nm + '_col', col.ctypes.data if len(col) else None); setattr(st, nm + '_val', None)
    return st, keep, [k[2].ctypes.data if len(k[2]) else None for k in keep]


def plan_struct(lib, st, copies=1, cidx=(None, None, None), table=None):
    """the plan of the system `st` (an fk_r1cs; coefficients from its values, or coded: cidx pointers and table, (n, 4) uint64 Montgomery with
    table[0] = ONE) as a dict: lists / lists_dd per matrix (None where there is none), segs / segs_dd (PlanSegs.table()), aliases as
    fk_r1cs_aliases' tuples, the query lists, and the PlanInfo for the rest"""
    gates = int(st.num_gates)
    nv = 1 + copies * (st.num_input - 1) + copies * st.num_aux
    if table is not None:
        table = np.ascontiguousarray(table, np.uint64).reshape(-1, 4)
    info = PlanInfo()
    lists = [np.full(max(gates, 1), 0xffffffff, np.uint32) for _ in range(3)]
    lists_dd = [np.full(max(gates, 1), 0xffffffff, np.uint32) for _ in range(3)]
    al = [np.zeros(max(3 * gates, 1), np.uint32) for _ in range(4)]
    idx = [np.zeros(max(nv, 1), np.uint32) for _ in range(2)]
    for k in range(3):
        info.list[k], info.list_dd[k] = lists[k].ctypes.data, lists_dd[k].ctypes.data
    info.alias_dst_mtx, info.alias_dst_row, info.alias_src_mtx, info.alias_src_row = (a.ctypes.data for a in al)
    info.idx_a, info.idx_b = idx[0].ctypes.data, idx[1].ctypes.data
    rc, err = plan_host_raw(lib, st, copies, cidx, table.ctypes.data if table is not None else None, len(table) if table is not None else 0, info)
    assert rc == 0, (rc, err)
    n = int(info.n_alias)
    return {
        'info': info,
        'lists': [lists[k][:gates] if (info.segs.mask >> k) & 1 else None for k in range(3)],
        'lists_dd': [lists_dd[k][:info.n_dd[k]] if info.own_dd[k] else None for k in range(3)],
        'segs': info.segs.table(), 'segs_dd': info.segs_dd.table(),
        'aliases': list(zip(*(a[:n].tolist() for a in al))) if n else [],
        'idx_a': idx[0][:info.n_idx_a], 'idx_b': idx[1][:info.n_idx_b],
        'win_cnt': np.ctypeslib.as_array(info.win_cnt).copy(), 'win_cnt_dd': np.ctypeslib.as_array(info.win_cnt_dd).copy(),
    }


def plan_host(lib, num_input, num_aux, mats, table, copies=1):
    """plan_struct of the coded system mats = three (ptr u64, col u32, cidx u32) over `table`"""
    st, keep, cidx = coded_struct(num_input, num_aux, mats)
    return plan_struct(lib, st, copies, cidx, table)
