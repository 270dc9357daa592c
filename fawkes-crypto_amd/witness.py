"""
Device witness generation (include/fawkes_hip_witness.h, csrc/witness.hip): the witness program of ONE instance of a batch circuit,
built here as data, checked on the host, interpreted on the GPU once per copy.

What the reference computes by re-running the circuit closure on `WitnessCS` for every proof (prover.rs:69-76) is, for a gadget without
data-dependent control flow, a straight-line program: every auxiliary variable is GIVEN (a caller-supplied value), MUL / DIV0 / INV0 of
linear combinations of earlier variables, or a BIT of one.  `WitnessProgram` builds such a program and runs it in Python integers
(`run_host`: the reference the device is compared with); `load` makes it resident; `generate` / `generate_dev` run it on `copies` given
rows and leave the witness in the tiled variable order of `Context.load_r1cs(..., copies=)`; `prove_given` goes from the given rows to the
256 proof bytes with no host witness in between.

The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
Limits: one GPU; the tiled order only; `assert_nonzero`'s hint (`unwrap_or(ONE)`, num.rs:49-62) is not an opcode; the given rows (roots,
signatures, cofactor preimages) are the caller's, who can compute them with the device Poseidon and JubJub calls of api.py.
"""
import ctypes as C

import numpy as np

from . import api
from .api import FR_MODULUS, FkError, _Handle, _check

GIVEN, MUL, DIV0, INV0, BIT = range(5)
OP_NAMES = ('GIVEN', 'MUL', 'DIV0', 'INV0', 'BIT')

I, U32, P = C.c_int, C.c_uint32, C.c_void_p


class WitnessDesc(C.Structure):
    """fk_witness_desc"""
    _fields_ = [('num_input', U32), ('num_aux', U32), ('n_given', U32), ('n_lc', U32),
                ('op', P), ('arg0', P), ('arg1', P), ('input_lc', P), ('lc_ptr', P), ('lc_col', P), ('lc_val', P)]


DESC = C.POINTER(WitnessDesc)

# one prototype per function of include/fawkes_hip_witness.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_witness_program_check': (I, (DESC,)),
    'fk_witness_program_load': (I, (P, DESC, P)),
    'fk_witness_program_info': (I, (P, P)),
    'fk_witness_program_free': (None, (P, P)),
    'fk_witness_generate_dev': (I, (P, P, P, U32, P)),
    'fk_witness_generate': (I, (P, P, P, U32, P)),
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


class WitnessProgram:
    """The witness program of one instance.  Variables are numbered in allocation order (Aux(0), Aux(1), ...); a linear combination is a
    sequence of (column, coefficient) with column 0 = ONE and 1 + j = Aux(j), coefficients canonical ints; `lc` returns its index and
    stores equal combinations once."""

    def __init__(self):
        self.num_input = 1
        self.n_given = 0
        self.op, self.arg0, self.arg1 = [], [], []
        self.input_lc = []
        self.lcs = []
        self._lc_index = {}

    num_aux = property(lambda self: len(self.op))

    def lc(self, terms):
        key = tuple((int(c), int(k) % FR_MODULUS) for c, k in terms)
        i = self._lc_index.get(key)
        if i is None:
            i = self._lc_index[key] = len(self.lcs)
            self.lcs.append(key)
        return i

    def _push(self, op, a0, a1=0):
        self.op.append(op); self.arg0.append(int(a0)); self.arg1.append(int(a1))
        return len(self.op) - 1

    def given(self):
        """the next element of the copy's given row"""
        self.n_given += 1
        return self._push(GIVEN, self.n_given - 1)

    def mul(self, la, lb):
        return self._push(MUL, la, lb)

    def div0(self, la, lb):
        return self._push(DIV0, la, lb)

    def inv0(self, la):
        return self._push(INV0, la)

    def bit(self, la, i):
        return self._push(BIT, la, i)

    def public(self, la):
        """the next public input is the combination la (`inputize`)"""
        self.input_lc.append(int(la))
        self.num_input += 1

    def counts(self):
        """operations by kind, and the runs of consecutive BITs that share one combination"""
        out = {n: self.op.count(k) for k, n in enumerate(OP_NAMES)}
        out['BIT_runs'] = sum(1 for v, k in enumerate(self.op)
                              if k == BIT and not (v and self.op[v - 1] == BIT and self.arg0[v - 1] == self.arg0[v]))
        return out

    def desc(self, explicit_ones=False):
        """the fk_witness_desc of this program; lc_val is NULL when every coefficient is ONE (unless explicit_ones).  The arrays it
        points into stay alive with the returned object (`.keep`)."""
        ptr = np.zeros(len(self.lcs) + 1, np.uint64)
        if self.lcs:
            ptr[1:] = np.cumsum([len(l) for l in self.lcs])
        nnz = int(ptr[-1])
        col = np.fromiter((c for l in self.lcs for c, _ in l), np.uint32, nnz)
        val = None
        if explicit_ones or any(k != 1 for l in self.lcs for _, k in l):
            cache, val = {}, np.zeros((nnz, 4), np.uint64)
            i = 0
            for l in self.lcs:
                for _, k in l:
                    m = cache.get(k)
                    if m is None:
                        m = cache[k] = api.int_to_limbs((k << 256) % FR_MODULUS)
                    val[i] = m
                    i += 1
        d = WitnessDesc()
        d.keep = [np.asarray(self.op, np.uint8), np.asarray(self.arg0, np.uint32), np.asarray(self.arg1, np.uint32),
                  np.asarray(self.input_lc, np.uint32), ptr, col, val]
        d.num_input, d.num_aux, d.n_given, d.n_lc = self.num_input, self.num_aux, self.n_given, len(self.lcs)
        for name, arr in zip(('op', 'arg0', 'arg1', 'input_lc', 'lc_ptr', 'lc_col', 'lc_val'), d.keep):
            setattr(d, name, arr.ctypes.data if arr is not None and arr.size else None)
        d.lc_ptr = ptr.ctypes.data
        return d

    def run_host(self, given_rows):
        """The program in Python integers: the tiled witness of len(given_rows) copies as canonical ints -- ONE, every copy's inputs,
        every copy's aux.  `api._fr_rows` of it is what the device writes."""
        ins, auxs = [], []
        for row in given_rows:
            row = [int(x) % FR_MODULUS for x in row]
            if len(row) != self.n_given:
                raise ValueError('a given row holds %d values, the program takes %d' % (len(row), self.n_given))
            z = []

            def ev(l):
                return sum(k * (z[c - 1] if c else 1) for c, k in self.lcs[l]) % FR_MODULUS

            held = (None, 0)                # the combination of the current run of BITs and its canonical value
            for v, (op, a0, a1) in enumerate(zip(self.op, self.arg0, self.arg1)):
                if op == BIT:
                    if not (v and self.op[v - 1] == BIT and held[0] == a0):
                        held = (a0, ev(a0))
                    z.append((held[1] >> a1) & 1)
                    continue
                if op == GIVEN:
                    z.append(row[a0])
                elif op == MUL:
                    z.append(ev(a0) * ev(a1) % FR_MODULUS)
                elif op == DIV0:
                    z.append(ev(a0) * pow(ev(a1), FR_MODULUS - 2, FR_MODULUS) % FR_MODULUS)
                elif op == INV0:
                    z.append(pow(ev(a0), FR_MODULUS - 2, FR_MODULUS))
                else:
                    raise ValueError('variable %d: unknown opcode %r' % (v, op))
            ins.append([ev(l) for l in self.input_lc])
            auxs.append(z)
        return [1] + [x for r in ins for x in r] + [x for r in auxs for x in r]

    def witness_len(self, copies):
        return 1 + copies * (self.num_input - 1) + copies * self.num_aux


def check(program):
    """fk_witness_program_check: raises FkError (FK_ERR_BAD_ARG, or FK_ERR_FORMAT for a coefficient image not below r) naming the
    offending variable or combination.  Host only.  `program`: a WitnessProgram or a WitnessDesc."""
    lib = _lib()
    d = program.desc() if isinstance(program, WitnessProgram) else program
    _check(lib.fk_witness_program_check(C.byref(d)), 'fk_witness_program_check', lib.fk_last_error, None)


class DeviceWitnessProgram(_Handle):
    """A witness program resident in device memory (fk_witness_program_load)."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle
        i = self.info()
        self.num_input, self.num_aux, self.n_given = i['num_input'], i['num_aux'], i['n_given']

    def info(self):
        out = (C.c_uint64 * 8)()
        _check(_lib().fk_witness_program_info(self.handle, out), 'fk_witness_program_info')
        return dict(zip(('num_input', 'num_aux', 'n_given', 'lcs', 'lc_terms', 'distinct_coefficients', 'lc_evaluations', 'inversions'), (int(x) for x in out)))

    def witness_len(self, copies):
        return 1 + copies * (self.num_input - 1) + copies * self.num_aux

    def _release(self, h):
        if self.ctx.handle:             # a closed context has released its device memory itself
            _lib().fk_witness_program_free(self.ctx.handle, h)


def load(ctx, program):
    """fk_witness_program_load: checks, dictionary-codes and uploads; an invalid program raises FkError and nothing reaches the device"""
    lib = _lib()
    d = program.desc() if isinstance(program, WitnessProgram) else program
    h = C.c_void_p()
    ctx._ck(lib.fk_witness_program_load(ctx.handle, C.byref(d), C.byref(h)))
    return DeviceWitnessProgram(ctx, h)


def _given_rows(prog, given):
    """(copies, the rows as (copies * n_given, 4) Montgomery limbs); every value is checked to be below r -- the device does not"""
    if isinstance(given, np.ndarray) and given.dtype == np.uint64:
        a = np.ascontiguousarray(given).reshape(-1, 4)
        below = np.zeros(len(a), bool)
        undecided = np.ones(len(a), bool)
        for j, q in zip(range(3, -1, -1), reversed(api.int_to_limbs(FR_MODULUS))):
            below |= undecided & (a[:, j] < q)
            undecided &= a[:, j] == q
        if not below.all():
            raise ValueError('given value %d is not below the modulus' % int(np.argmin(below)))
        copies = len(a) // prog.n_given if prog.n_given else None
    else:
        copies = len(given)
        a = api._fr_rows([x for row in given for x in row], copies * prog.n_given)
    if copies is None or len(a) != copies * prog.n_given:
        raise ValueError('the given rows hold %d values: not a multiple of the program\'s %d' % (len(a), prog.n_given))
    return copies, a


def generate_dev(ctx, prog, d_given, copies, d_z):
    """fk_witness_generate_dev: device pointers; asynchronous on the library's stream, so a prove_witness_dev on d_z needs no sync"""
    ctx._ck(_lib().fk_witness_generate_dev(ctx.handle, prog.handle, d_given, int(copies), d_z))


def generate(ctx, prog, given):
    """fk_witness_generate: `given` = one row of n_given values per copy (canonical ints, or a Montgomery limb array) -> the tiled
    witness, (witness_len(copies), 4) uint64 Montgomery"""
    copies, a = _given_rows(prog, given)
    z = np.zeros((prog.witness_len(copies) if copies else 0, 4), np.uint64)
    ctx._ck(_lib().fk_witness_generate(ctx.handle, prog.handle, api._vp(a) if a.size else None, copies, api._vp(z) if z.size else None))
    return z


def prove_given(ctx, key, device_r1cs, prog, given, r, s, want_timings=False):
    """From the circuit's secret inputs to the proof: uploads the given rows, generates the witness on the device and hands it to
    fk_prove_r1cs_dev on the same stream -- no host witness in between.  device_r1cs: Context.load_r1cs(instance, copies=len(given))."""
    copies, a = _given_rows(prog, given)
    n = prog.witness_len(copies)
    nv = device_r1cs.info()['num_vars']
    if n != nv:
        raise FkError(6, 'the program writes %d field elements for %d copies, the constraint system has %d variables' % (n, copies, nv))
    d_given, d_z = ctx.dev_alloc(max(a.nbytes, 32)), ctx.dev_alloc(32 * n)
    try:
        if a.size:
            ctx.upload(d_given, a)
        generate_dev(ctx, prog, d_given, copies, d_z)
        return ctx.prove_witness_dev(key, device_r1cs, d_z, r, s, want_timings)
    finally:
        ctx.dev_free(d_given)
        ctx.dev_free(d_z)
