"""
Batch prover (include/fawkes_hip_batch.h, csrc/batch_prove.hip): `count` Groth16 proofs of ONE small circuit under ONE key in one call.

`prove_batch` takes the witnesses as host rows, `prove_batch_dev` as a device array in either layout (ROWS: one row per proof; TILED: the
order `witness.generate_dev` writes for `count` copies), `prove_given_batch` goes from the circuits' secret inputs to `count` independent
proofs of the ONE-instance key with no host copy of the witness.  Proof i is byte for byte `Context.prove_witness` of witness i with
(r_i, s_i).  `plan` says, without a GPU, how a call is cut into groups; `r1cs_eval_dev`, `quotient_dev` and `msm_dev` run one stage alone.

The per-proof R1CS check (include/fawkes_hip_batch_check.h, csrc/batch_check.hip): `check_batch` / `check_batch_dev` evaluate and judge
`count` witnesses with no key; `prove_batch_checked`, `prove_batch_checked_dev` and `prove_given_batch_checked` return the bytes of the
unchecked calls plus one `check.CheckReport` per proof, made from the evaluation the proofs are made from; `check_batch_host` is the host
reference (no GPU).  A violated witness is no error unless `raise_on_bad=True`, which raises `BatchUnsatisfied`.

The C prototypes of these entry points live in this module's own tables, one per header (the table of _abi.py mirrors fawkes_hip.h and
nothing else).
Limits: one GPU, an unsharded key, an explicit (not tiled) resident system, domains up to 2^20.
"""
import ctypes as C

import numpy as np

from . import api
from . import check as _check_mod
from . import witness as _witness
from .api import FK_PROOF_BYTES, FkError, _check, _fr, _vp

Z_ROWS, Z_TILED = 0, 1
MAX_LOG_M = 20
WINDOW_BITS_MIN, WINDOW_BITS_MAX = 2, 14
MAX_GROUP = 32768
PLAN_DEFAULT_BUDGET = 16 << 30
CHECK_LAUNCHES = 4              # FK_BATCH_CHECK_LAUNCHES
CHECK_RECORD_BYTES = 160        # FK_BATCH_CHECK_RECORD_BYTES

I, U32, U64, P = C.c_int, C.c_uint32, C.c_uint64, C.c_void_p


class BatchOpts(C.Structure):
    """fk_batch_opts"""
    _fields_ = [('scratch_budget_bytes', U64), ('window_bits_g1', U32), ('window_bits_g2', U32)]


class BatchPlanInfo(C.Structure):
    """fk_batch_plan_info"""
    _fields_ = [('group', U32), ('n_groups', U32), ('window_bits_g1', U32), ('windows_g1', U32), ('window_bits_g2', U32), ('windows_g2', U32),
                ('segment', U32), ('ntt_passes', U32), ('launches_per_group', U32), ('reserved', U32), ('scratch_bytes', U64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != 'reserved'}


class BatchTimings(C.Structure):
    """fk_batch_timings"""
    _fields_ = [(n, C.c_double) for n in ('eval_ms', 'quotient_ms', 'msm_h_ms', 'msm_l_ms', 'msm_a_ms', 'msm_b1_ms', 'msm_b2_ms', 'assemble_ms', 'total_ms')]

    def as_dict(self):
        return {n: float(getattr(self, n)) for n, _ in self._fields_}


OPTS, PLAN, TIMINGS = C.POINTER(BatchOpts), C.POINTER(BatchPlanInfo), C.POINTER(BatchTimings)

# one prototype per function of include/fawkes_hip_batch.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_prove_batch_plan': (I, (U64, U64, U64, U64, U32, OPTS, PLAN)),
    'fk_prove_batch_dev': (I, (P, P, P, P, I, U32, P, P, P, OPTS, TIMINGS)),
    'fk_prove_batch': (I, (P, P, P, P, U32, P, P, P, OPTS, TIMINGS)),
    'fk_batch_r1cs_eval_dev': (I, (P, P, P, I, U32, P, P, P)),
    'fk_batch_quotient_dev': (I, (P, P, P, P, U64, U32, U32, P)),
    'fk_batch_msm_dev': (I, (P, P, U64, I, P, U32, P, I, U32, U32, U32, OPTS, P)),
}

REPORTS, F64P = C.POINTER(_check_mod.CheckReportStruct), C.POINTER(C.c_double)

# one prototype per function of include/fawkes_hip_batch_check.h
CHECK_PROTOTYPES = {
    'fk_batch_r1cs_check': (I, (P, P, P, I, U32, P, P, REPORTS)),
    'fk_batch_r1cs_check_dev': (I, (P, P, P, I, U32, P, P, REPORTS, OPTS)),
    'fk_prove_batch_checked_dev': (I, (P, P, P, P, I, U32, P, P, P, OPTS, TIMINGS, P, P, REPORTS, F64P)),
    'fk_prove_batch_checked': (I, (P, P, P, P, U32, P, P, P, OPTS, TIMINGS, P, P, REPORTS, F64P)),
}

_APPLIED = None


def _lib():
    """the loaded library with this module's prototypes applied (once)"""
    global _APPLIED
    lib = api.load_library()
    if _APPLIED is not lib:
        for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(CHECK_PROTOTYPES.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        _APPLIED = lib
    return lib


def _opts(opts):
    """None | BatchOpts | dict(scratch_budget_bytes=, window_bits_g1=, window_bits_g2=) -> a pointer argument (and what keeps it alive)"""
    if opts is None:
        return None
    if isinstance(opts, dict):
        opts = BatchOpts(**opts)
    return C.byref(opts)


def plan(m, n_l, n_a, n_b, count, opts=None):
    """fk_prove_batch_plan (host only): how `count` proofs of a key with domain m and these query lengths are cut into groups"""
    lib = _lib()
    info = BatchPlanInfo()
    _check(lib.fk_prove_batch_plan(int(m), int(n_l), int(n_a), int(n_b), int(count), _opts(opts), C.byref(info)), 'fk_prove_batch_plan', lib.fk_last_error, None)
    return info.as_dict()


def _rs(rs, ss, count):
    r, s = _fr(np.asarray(rs, np.uint64).reshape(-1, 4), count), _fr(np.asarray(ss, np.uint64).reshape(-1, 4), count)
    return r, s


def prove_batch_dev(ctx, key, dr, d_z, layout, count, rs, ss, opts=None, want_timings=False):
    """fk_prove_batch_dev: the witnesses on the device in `layout` (Z_ROWS / Z_TILED) -> (count, 256) uint8"""
    count = int(count)
    r, s = _rs(rs, ss, count)
    out = np.zeros((count, FK_PROOF_BYTES), np.uint8)
    tm = BatchTimings()
    ctx._ck(_lib().fk_prove_batch_dev(ctx.handle, key.handle, dr.handle, d_z, int(layout), count, _vp(r) if count else None, _vp(s) if count else None,
                                      _vp(out) if count else None, _opts(opts), C.byref(tm)))
    return (out, tm.as_dict()) if want_timings else out


def prove_batch(ctx, key, dr, zs, rs, ss, opts=None, want_timings=False):
    """fk_prove_batch: zs = count witnesses, (count, num_input + num_aux, 4) uint64 Montgomery, each with its own ONE -> (count, 256) uint8"""
    z = np.ascontiguousarray(zs, np.uint64)
    count = z.shape[0] if z.ndim == 3 else len(zs)
    nv = dr.info()['num_vars']
    if z.size != count * nv * 4:
        raise FkError(6, 'the witnesses hold %d field elements, %d proofs of a system of %d variables take %d' % (z.size // 4, count, nv, count * nv))
    r, s = _rs(rs, ss, count)
    out = np.zeros((count, FK_PROOF_BYTES), np.uint8)
    tm = BatchTimings()
    ctx._ck(_lib().fk_prove_batch(ctx.handle, key.handle, dr.handle, _vp(z) if count else None, count, _vp(r) if count else None, _vp(s) if count else None,
                                  _vp(out) if count else None, _opts(opts), C.byref(tm)))
    return (out, tm.as_dict()) if want_timings else out


def prove_given_batch(ctx, prog, key, dr, given, rs, ss, opts=None, want_timings=False):
    """From the circuits' secret inputs to `count` independent proofs of the ONE-instance key: uploads the given rows, generates the
    witnesses on the device (witness.generate_dev, tiled order) and hands them to fk_prove_batch_dev on the same stream -- no host witness in
    between.  prog: witness.load(...); dr: Context.load_r1cs(instance) (NOT copies=: that would be one proof of a count-fold circuit)."""
    copies, a = _witness._given_rows(prog, given)
    n = prog.witness_len(copies)
    nv = dr.info()['num_vars']
    if prog.num_input + prog.num_aux != nv:
        raise FkError(6, 'the program writes %d variables per copy, the constraint system has %d' % (prog.num_input + prog.num_aux, nv))
    d_given, d_z = ctx.dev_alloc(max(a.nbytes, 32)), ctx.dev_alloc(32 * max(n, 1))
    try:
        if a.size:
            ctx.upload(d_given, a)
        _witness.generate_dev(ctx, prog, d_given, copies, d_z)
        return prove_batch_dev(ctx, key, dr, d_z, Z_TILED, copies, rs, ss, opts, want_timings)
    finally:
        ctx.dev_free(d_given)
        ctx.dev_free(d_z)


def r1cs_eval_dev(ctx, dr, d_z, layout, count, d_a, d_b, d_c):
    """fk_batch_r1cs_eval_dev: a, b, c of `count` witnesses, count x next_pow2(rows) elements each"""
    ctx._ck(_lib().fk_batch_r1cs_eval_dev(ctx.handle, dr.handle, d_z, int(layout), int(count), d_a, d_b, d_c))


def quotient_dev(ctx, d_a, d_b, d_c, n_rows, log_m, count, d_h):
    """fk_batch_quotient_dev: the quotients of `count` rows of a, b, c (count x 2^log_m each; all three are used as scratch)"""
    ctx._ck(_lib().fk_batch_quotient_dev(ctx.handle, d_a, d_b, d_c, int(n_rows), int(log_m), int(count), d_h))


def msm_dev(ctx, d_bases, n, g2, d_z, layout, z_vars, count, d_idx=None, var_offset=0, num_input=1, opts=None):
    """fk_batch_msm_dev: `count` multiplications over shared bases -> (count, 64 or 128) uint8 raw affine"""
    out = np.zeros((int(count), 128 if g2 else 64), np.uint8)
    ctx._ck(_lib().fk_batch_msm_dev(ctx.handle, d_bases, int(n), 1 if g2 else 0, d_idx, int(var_offset), d_z, int(layout), int(num_input), int(z_vars), int(count),
                                    _opts(opts), _vp(out) if count else None))
    return out


# ---------------------------------------------------------------- the per-proof check
class BatchUnsatisfied(RuntimeError):
    """raised by the checked prove wrappers under raise_on_bad=True; `.reports` are all the CheckReports, `.bad` the indices of the proofs
    whose report is not ok, `.proofs` the proofs that were made anyway"""

    def __init__(self, reports, bad, proofs=None):
        RuntimeError.__init__(self, '%d of %d witnesses violate the constraint system: proofs %s' % (len(bad), len(reports), bad[:16]))
        self.reports, self.bad, self.proofs = reports, bad, proofs


def _reports(sts, bitmaps):
    """report structs and the (count, words) bitmap (None: nothing was bad, nothing was downloaded) -> CheckReports"""
    return [_check_mod.CheckReport(st, 0, np.array(bitmaps[i]) if bitmaps is not None and st.n_bad > 0 else None) for i, st in enumerate(sts)]


def _host_witnesses(nv, zs, layout, count):
    """the witnesses as one contiguous array and how many they are (derived from the length where count is None)"""
    z = np.ascontiguousarray(zs, np.uint64)
    if count is None:
        if layout == Z_ROWS:
            count = z.shape[0] if z.ndim == 3 else z.size // (4 * nv)
        else:
            count = (z.size // 4 - 1) // (nv - 1) if nv > 1 else 1
    n = count * nv if layout == Z_ROWS else 1 + count * (nv - 1)
    if count and z.size != n * 4:
        raise FkError(6, 'the witnesses hold %d field elements, %d proofs of a system of %d variables take %d' % (z.size // 4, count, nv, n))
    return z, int(count)


def check_batch_host(r1cs, zs, layout=Z_ROWS, count=None):
    """fk_batch_r1cs_check: the host reference, no GPU.  r1cs: an `R1cs`, ONE instance; zs: the witnesses as (count, num_vars, 4) uint64
    Montgomery rows (Z_ROWS) or in the tiled order (Z_TILED; count is then derived from the length unless given).  Returns a list of
    `check.CheckReport`, one per proof."""
    lib = _lib()
    z, count = _host_witnesses(r1cs.num_input + r1cs.num_aux, zs, layout, count)
    words = (r1cs.num_gates + 63) // 64
    bitmaps = np.zeros((count, words), np.uint64)
    sts = (_check_mod.CheckReportStruct * max(count, 1))()
    _check(lib.fk_batch_r1cs_check(None, C.byref(r1cs.struct), _vp(z) if count else None, int(layout), count, _vp(bitmaps) if bitmaps.size else None, None, sts),
           'fk_batch_r1cs_check', lib.fk_last_error, None)
    return _reports(sts[:count], bitmaps)


class _BatchOutputs:
    """the device bitmap and flags and the host reports of one call; the bitmap is downloaded only when a gate is bad"""

    def __init__(self, ctx, dr, count):
        self.ctx, self.count = ctx, int(count)
        self.sts = (_check_mod.CheckReportStruct * max(self.count, 1))()
        words = (dr.info()['rows'] + 63) // 64                    # gates <= rows: certainly enough
        self.d_bitmap = ctx.dev_alloc(max(8 * words * self.count, 8))
        self.d_bad = None
        try:
            self.d_bad = ctx.dev_alloc(max(self.count, 8))
        except Exception:
            self.free()
            raise

    def reports(self):
        sts, bitmaps = self.sts[:self.count], None
        if any(st.n_bad > 0 for st in sts):
            words = (int(sts[0].gates) + 63) // 64
            bitmaps = self.ctx.download(self.d_bitmap, 8 * words * self.count, np.uint64).reshape(self.count, words)
        return _reports(sts, bitmaps)

    def proof_bad(self):
        """the device flags as numpy (count,) uint8"""
        return self.ctx.download(self.d_bad, self.count, np.uint8) if self.count else np.zeros(0, np.uint8)

    def free(self):
        for p in (self.d_bitmap, self.d_bad):
            if p:
                self.ctx.dev_free(p)
        self.d_bitmap = self.d_bad = None


def check_batch_dev(ctx, dr, d_z, layout, count, opts=None):
    """fk_batch_r1cs_check_dev: evaluates and checks `count` witnesses on the device in `layout`, no key and no proof -> list of
    `check.CheckReport`.  opts: scratch_budget_bytes cuts the call into groups."""
    out = _BatchOutputs(ctx, dr, count)
    try:
        ctx._ck(_lib().fk_batch_r1cs_check_dev(ctx.handle, dr.handle, d_z, int(layout), out.count, out.d_bitmap, out.d_bad, out.sts, _opts(opts)))
        return out.reports()
    finally:
        out.free()


def check_batch(ctx, dr, zs, opts=None):
    """check_batch_dev of host witnesses, (count, num_vars, 4) uint64 Montgomery rows, each with its own ONE (uploaded)"""
    nv = dr.info()['num_vars']
    z, count = _host_witnesses(nv, zs, Z_ROWS, None)
    d_z = ctx.dev_alloc(max(z.nbytes, 32))
    try:
        if z.nbytes:
            ctx.upload(d_z, z)
        return check_batch_dev(ctx, dr, d_z, Z_ROWS, count, opts)
    finally:
        ctx.dev_free(d_z)


def _checked_result(out, proofs, tm, check_ms, raise_on_bad, want_timings):
    reports = out.reports()
    if raise_on_bad:
        bad = [i for i, rep in enumerate(reports) if not rep.ok]
        if bad:
            raise BatchUnsatisfied(reports, bad, proofs)
    if want_timings:
        return proofs, reports, dict(tm.as_dict(), check_ms=float(check_ms.value))
    return proofs, reports


def prove_batch_checked_dev(ctx, key, dr, d_z, layout, count, rs, ss, opts=None, raise_on_bad=False, want_timings=False):
    """fk_prove_batch_checked_dev: the bytes of prove_batch_dev and one CheckReport per proof, from the same evaluation.  Returns
    (proofs, reports), or (proofs, reports, timings) where timings has the stages of prove_batch_dev plus `check_ms`.
    raise_on_bad: raise BatchUnsatisfied (carrying reports, indices and proofs) unless every report is ok."""
    count = int(count)
    r, s = _rs(rs, ss, count)
    proofs = np.zeros((count, FK_PROOF_BYTES), np.uint8)
    tm, check_ms = BatchTimings(), C.c_double(0)
    out = _BatchOutputs(ctx, dr, count)
    try:
        ctx._ck(_lib().fk_prove_batch_checked_dev(ctx.handle, key.handle, dr.handle, d_z, int(layout), count, _vp(r) if count else None, _vp(s) if count else None,
                                                  _vp(proofs) if count else None, _opts(opts), C.byref(tm), out.d_bitmap, out.d_bad, out.sts,
                                                  C.byref(check_ms) if want_timings else None))
        return _checked_result(out, proofs, tm, check_ms, raise_on_bad, want_timings)
    finally:
        out.free()


def prove_batch_checked(ctx, key, dr, zs, rs, ss, opts=None, raise_on_bad=False, want_timings=False):
    """fk_prove_batch_checked: prove_batch plus one CheckReport per proof; returns as prove_batch_checked_dev does"""
    z, count = _host_witnesses(dr.info()['num_vars'], zs, Z_ROWS, None)
    r, s = _rs(rs, ss, count)
    proofs = np.zeros((count, FK_PROOF_BYTES), np.uint8)
    tm, check_ms = BatchTimings(), C.c_double(0)
    out = _BatchOutputs(ctx, dr, count)
    try:
        ctx._ck(_lib().fk_prove_batch_checked(ctx.handle, key.handle, dr.handle, _vp(z) if count else None, count, _vp(r) if count else None, _vp(s) if count else None,
                                              _vp(proofs) if count else None, _opts(opts), C.byref(tm), out.d_bitmap, out.d_bad, out.sts,
                                              C.byref(check_ms) if want_timings else None))
        return _checked_result(out, proofs, tm, check_ms, raise_on_bad, want_timings)
    finally:
        out.free()


def prove_given_batch_checked(ctx, prog, key, dr, given, rs, ss, opts=None, raise_on_bad=False, want_timings=False):
    """prove_given_batch plus the verdicts: given rows -> device witness (witness.generate_dev, tiled order) -> fk_prove_batch_checked_dev on
    the same stream, no host witness in between.  Returns as prove_batch_checked_dev does; report i speaks of given row i."""
    copies, a = _witness._given_rows(prog, given)
    n = prog.witness_len(copies)
    nv = dr.info()['num_vars']
    if prog.num_input + prog.num_aux != nv:
        raise FkError(6, 'the program writes %d variables per copy, the constraint system has %d' % (prog.num_input + prog.num_aux, nv))
    d_given, d_z = ctx.dev_alloc(max(a.nbytes, 32)), ctx.dev_alloc(32 * max(n, 1))
    try:
        if a.size:
            ctx.upload(d_given, a)
        _witness.generate_dev(ctx, prog, d_given, copies, d_z)
        return prove_batch_checked_dev(ctx, key, dr, d_z, Z_TILED, copies, rs, ss, opts, raise_on_bad, want_timings)
    finally:
        ctx.dev_free(d_given)
        ctx.dev_free(d_z)
