"""
The R1CS check (include/fawkes_hip_check.h, csrc/check.hip): which gates, and which copies of a batch circuit, a witness violates.

The prover's bytes are defined for any witness: a bad signature is proved like any other and the proof then fails to verify, which says
that something is wrong and not what.  `check_witness` evaluates a = A z, b = B z, c = C z on the device with the prover's own evaluator
and tests a * b == c per gate; `prove_checked` does so on the very evaluation a proof is made from, between the evaluation and the
quotient; `prove_given_checked` goes from the given rows of a batch to the proof and the list of bad copies; `check_host` is the plain
host reference (no GPU) the device is compared with.  A violated system is no error: the calls return and the `CheckReport` speaks --
unless `raise_on_bad=True` is passed to a prove wrapper, which then raises `Unsatisfied`.

The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
Limits: one GPU; the witness on the device (the host-witness and the submit / wait paths are not checked); a gate is named, not the
variable that breaks it.
"""
import ctypes as C

import numpy as np

from . import api, witness
from .api import FK_PROOF_BYTES, FkError, _fr, _vp
from ._abi import Timings

CHECK_NONE = (1 << 64) - 1

I, U32, U64, P = C.c_int, C.c_uint32, C.c_uint64, C.c_void_p


class CheckReportStruct(C.Structure):
    """fk_check_report"""
    _fields_ = [('gates', U64), ('n_bad', U64), ('first_bad', U64), ('first_abc', U64 * 4 * 3), ('n_groups', U64), ('n_bad_groups', U64),
                ('n_range', U64), ('first_range', U64), ('one_ok', C.c_int32), ('gates_valid', C.c_int32)]


# one prototype per function of include/fawkes_hip_check.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_r1cs_check': (I, (P, P, U32, P, U64, P, P, P)),
    'fk_r1cs_check_dev': (I, (P, P, P, U64, P, P, P)),
    'fk_prove_r1cs_checked_dev': (I, (P, P, P, P, P, P, P, P, U64, P, P, P)),
}

_APPLIED = None


def _lib():
    """the loaded library with this module's prototypes applied (once)"""
    global _APPLIED
    lib = api.load_library()
    if _APPLIED is not lib:
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        _APPLIED = lib
    return lib


class CheckReport:
    """What a check found.  `first_bad` / `first_range` are None where the C report says FK_CHECK_NONE; `first_abc` are the canonical
    <A, z>, <B, z>, <C, z> of the lowest bad gate (None without one).  With `gates_valid` False (an element of the witness is not below
    r) the gate fields, `bad_rows()` and `bad_groups()` are unspecified."""

    def __init__(self, st, group_rows, bitmap=None, flags=None):
        self.gates, self.n_bad = int(st.gates), int(st.n_bad)
        self.first_bad = None if st.first_bad == CHECK_NONE else int(st.first_bad)
        self.first_abc_mont = np.array([[int(x) for x in row] for row in st.first_abc], np.uint64)
        self.first_abc = None if self.first_bad is None else tuple(api._fr_ints(self.first_abc_mont))
        self.group_rows = group_rows
        self.n_groups, self.n_bad_groups = int(st.n_groups), int(st.n_bad_groups)
        self.n_range = int(st.n_range)
        self.first_range = None if st.first_range == CHECK_NONE else int(st.first_range)
        self.one_ok, self.gates_valid = bool(st.one_ok), bool(st.gates_valid)
        self._bitmap, self._flags = bitmap, flags       # host copies; None where nothing was bad (nothing was downloaded)

    @property
    def ok(self):
        return self.gates_valid and self.one_ok and self.n_bad == 0 and self.n_range == 0

    def bitmap(self):
        """ceil(gates / 64) uint64 words, bit g % 64 of word g / 64 set iff gate g is bad"""
        if self._bitmap is None:
            return np.zeros((self.gates + 63) // 64, np.uint64)
        return self._bitmap

    def bad_rows(self):
        """the bad gates, ascending"""
        if self._bitmap is None:
            return np.zeros(0, np.int64)
        bits = np.unpackbits(self._bitmap.view(np.uint8), bitorder='little')
        return np.flatnonzero(bits).astype(np.int64)

    def group_flags(self):
        """n_groups bytes, 0 or 1"""
        if not self.group_rows:
            raise ValueError('the check ran without group_rows')
        if self._flags is None:
            return np.zeros(self.n_groups, np.uint8)
        return self._flags

    def bad_groups(self):
        """the groups (of group_rows consecutive gates: the copies of a tiled system) that hold a bad gate, ascending"""
        return np.flatnonzero(self.group_flags()).astype(np.int64)

    def __repr__(self):
        return 'CheckReport(gates=%d, n_bad=%d, first_bad=%r, n_bad_groups=%d/%d, n_range=%d, one_ok=%s, gates_valid=%s)' % (
            self.gates, self.n_bad, self.first_bad, self.n_bad_groups, self.n_groups, self.n_range, self.one_ok, self.gates_valid)


class Unsatisfied(RuntimeError):
    """raised by the prove wrappers under raise_on_bad=True; `.report` is the CheckReport, `.proof` the proof that was made anyway"""

    def __init__(self, report, proof=None):
        RuntimeError.__init__(self, 'the witness violates the constraint system: %r' % (report,))
        self.report, self.proof = report, proof


def _extents(rows, group_rows):
    """(bitmap words, group flags) that are certainly enough for a system of `rows` rows (gates <= rows)"""
    return (rows + 63) // 64, ((rows + group_rows - 1) // group_rows if group_rows else 0)


def check_host(r1cs, z, copies=1, group_rows=None):
    """fk_r1cs_check: the host reference, no GPU.  r1cs: an `R1cs`, ONE instance; z: the (tiled) witness of `copies` of it as (n, 4)
    uint64 Montgomery limbs.  Returns a CheckReport."""
    lib = _lib()
    z = _fr(z)
    copies, group_rows = int(copies), int(group_rows or 0)
    nv = 1 + copies * (r1cs.num_input - 1) + copies * r1cs.num_aux
    if copies >= 1 and len(z) != nv:
        raise FkError(6, 'witness holds %d field elements, %d copies of the constraint system have %d variables' % (len(z), copies, nv))
    words, groups = _extents(max(copies, 1) * r1cs.num_gates, group_rows)
    bitmap, flags = np.zeros(words, np.uint64), np.zeros(groups, np.uint8)
    st = CheckReportStruct()
    api._check(lib.fk_r1cs_check(None, C.byref(r1cs.struct), copies, _vp(z), group_rows, _vp(bitmap), _vp(flags) if group_rows else None, C.byref(st)),
               'fk_r1cs_check', lib.fk_last_error, None)
    bad = st.n_bad > 0
    return CheckReport(st, group_rows, bitmap if bad else None, flags[:int(st.n_groups)] if bad and group_rows else None)


class _DeviceOutputs:
    """the device bitmap and group flags of one call, downloaded only when a gate is bad"""

    def __init__(self, ctx, device_r1cs, group_rows):
        self.ctx, self.group_rows = ctx, int(group_rows or 0)
        words, groups = _extents(device_r1cs.info()['rows'], self.group_rows)
        self.d_bitmap = ctx.dev_alloc(max(8 * words, 8))
        self.d_flags = ctx.dev_alloc(max(groups, 8)) if self.group_rows else None
        self.st = CheckReportStruct()

    def report(self):
        st, bitmap, flags = self.st, None, None
        if st.n_bad > 0:
            bitmap = self.ctx.download(self.d_bitmap, 8 * ((int(st.gates) + 63) // 64), np.uint64)
            if self.group_rows:
                flags = self.ctx.download(self.d_flags, int(st.n_groups), np.uint8)
        return CheckReport(st, self.group_rows, bitmap, flags)

    def free(self):
        for p in (self.d_bitmap, self.d_flags):
            if p:
                self.ctx.dev_free(p)
        self.d_bitmap = self.d_flags = None


def check_witness(ctx, device_r1cs, z, group_rows=None):
    """fk_r1cs_check_dev.  z: a host array ((num_vars, 4) uint64 Montgomery; uploaded) or a device pointer (int) to the witness as
    prove_witness_dev takes it.  group_rows: gates per group -- the gates of one instance of a tiled system give one flag per copy.
    Returns a CheckReport."""
    lib = _lib()
    d_z, own = z, False
    if isinstance(z, np.ndarray):
        z = _fr(z)
        device_r1cs.check_witness(z)
        d_z, own = ctx.dev_alloc(max(z.nbytes, 32)), True
    out = None
    try:
        if own:
            ctx.upload(d_z, z)
        out = _DeviceOutputs(ctx, device_r1cs, group_rows)
        ctx._ck(lib.fk_r1cs_check_dev(ctx.handle, device_r1cs.handle, d_z, out.group_rows, out.d_bitmap, out.d_flags, C.byref(out.st)))
        return out.report()
    finally:
        if out is not None:
            out.free()
        if own:
            ctx.dev_free(d_z)


def prove_checked(ctx, key, device_r1cs, d_z, r, s, group_rows=None, raise_on_bad=False, want_timings=False):
    """fk_prove_r1cs_checked_dev: the 256 bytes of prove_witness_dev and the CheckReport of the evaluation they were made from.
    Returns (proof, report), or (proof, report, timings).  raise_on_bad: raise Unsatisfied (carrying both) unless report.ok."""
    lib = _lib()
    proof = np.zeros(FK_PROOF_BYTES, np.uint8)
    tm = Timings()
    r, s = _fr(r, 1), _fr(s, 1)
    out = _DeviceOutputs(ctx, device_r1cs, group_rows)
    try:
        ctx._ck(lib.fk_prove_r1cs_checked_dev(ctx.handle, key.handle, device_r1cs.handle, d_z, _vp(r), _vp(s), _vp(proof), C.byref(tm),
                                              out.group_rows, out.d_bitmap, out.d_flags, C.byref(out.st)))
        report = out.report()
    finally:
        out.free()
    if raise_on_bad and not report.ok:
        raise Unsatisfied(report, proof)
    return (proof, report, tm.as_dict()) if want_timings else (proof, report)


def prove_given_checked(ctx, key, device_r1cs, prog, given, r, s, raise_on_bad=False):
    """From the circuit's secret inputs to the proof and the bad copies: uploads the given rows, generates the witness on the device
    (witness.generate_dev) and hands it to the checked prover on the same stream, with one group per copy -- `report.bad_groups()` are the
    copies whose rows violate the circuit.  device_r1cs: Context.load_r1cs(instance, copies=len(given)).  Returns (proof, report)."""
    copies, a = witness._given_rows(prog, given)
    n = prog.witness_len(copies)
    info = device_r1cs.info()
    if n != info['num_vars'] or not copies:
        raise FkError(6, 'the program writes %d field elements for %d copies, the constraint system has %d variables' % (n, copies, info['num_vars']))
    gates = info['rows'] - 1 - copies * (prog.num_input - 1)
    if gates <= 0 or gates % copies:
        raise FkError(6, 'the constraint system\'s %d gates are not %d copies of one instance' % (gates, copies))
    d_given, d_z = ctx.dev_alloc(max(a.nbytes, 32)), ctx.dev_alloc(32 * n)
    try:
        if a.size:
            ctx.upload(d_given, a)
        witness.generate_dev(ctx, prog, d_given, copies, d_z)
        return prove_checked(ctx, key, device_r1cs, d_z, r, s, group_rows=gates // copies, raise_on_bad=raise_on_bad)
    finally:
        ctx.dev_free(d_given)
        ctx.dev_free(d_z)
