"""
Aggregated Groth16 batch verification (include/fawkes_hip_verify.h, csrc/verify_agg.hip): `count` proofs of one key checked by
ONE pairing equation -- a random linear combination with secret nonzero 128-bit weights -- instead of one equation per proof.

`verify_aggregate` is the raw call: (accept, wellformed, report).  `verify_batch_aggregated` is what a service calls: it returns the same
bool array as `api.verify_batch`, always -- all True when the aggregate accepts, otherwise the per-proof kernel decides about the
well-formed proofs (the aggregate says THAT a batch holds a bad proof, not WHICH).

The weights must not be known to whoever made the proofs: leave `weights=None` (the library draws them from getrandom(2) per call)
outside tests.  With known weights a prover can submit proofs that are each invalid and whose errors cancel in the sum
(tests/test_verify_aggregate_host.py shows the attack with weights (1, 1)).

The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
"""
import ctypes as C

import numpy as np

from . import api
from .api import FK_PROOF_BYTES, _check, _vp

I, U32, Z, P = C.c_int, C.c_uint32, C.c_size_t, C.c_void_p


class AggReport(C.Structure):
    """fk_verify_agg_report"""
    _fields_ = [('count', C.c_uint32), ('n_wellformed', C.c_uint32), ('equation_ok', C.c_int32),
                ('sum_w', C.c_uint64 * 4), ('s_acc', C.c_uint8 * 64), ('s_c', C.c_uint8 * 64)]

    def as_dict(self):
        """sum_w as its four Montgomery limbs, the two points as their 64 raw bytes"""
        return dict(count=self.count, n_wellformed=self.n_wellformed, equation_ok=self.equation_ok,
                    sum_w=tuple(self.sum_w), s_acc=bytes(self.s_acc), s_c=bytes(self.s_c))


REPORT = C.POINTER(AggReport)
_SIG = (I, (P, P, Z, P, U32, P, U32, P, P, C.POINTER(C.c_int), REPORT))

# one prototype per function of include/fawkes_hip_verify.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_verify_aggregate': _SIG,
    'fk_verify_aggregate_dev': _SIG,
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


def _weights(weights, count):
    """None, or (count, 2) uint64 from ints below 2^128 / an array of that shape"""
    if weights is None:
        return None
    if isinstance(weights, np.ndarray) and weights.dtype == np.uint64:
        w = np.ascontiguousarray(weights).reshape(-1, 2)
    else:
        if any(int(x) < 0 or int(x) >> 128 for x in weights):
            raise ValueError('a weight is a 128-bit unsigned integer')
        w = np.array([[int(x) & (2 ** 64 - 1), int(x) >> 64] for x in weights], np.uint64).reshape(-1, 2)
    if len(w) != count:
        raise ValueError('%d weights for %d proofs' % (len(w), count))
    return w


def verify_aggregate(ctx, vk_borsh, inputs, proofs, weights=None):
    """fk_verify_aggregate_dev on `ctx`, or fk_verify_aggregate on the host when ctx is None (no GPU needed: the reference of the device
    entry).  inputs (count, n_inputs, 4) uint64 Montgomery, proofs (count, 256) uint8, as for `api.verify_batch`; weights: None (drawn by
    the library) or `count` nonzero integers below 2^128 -- tests only.  Returns (accept, wellformed bool array, AggReport)."""
    lib = _lib()
    vkb = np.frombuffer(bytes(vk_borsh), np.uint8)
    pr = np.ascontiguousarray(proofs, np.uint8).reshape(-1, FK_PROOF_BYTES)
    inp = np.ascontiguousarray(inputs, np.uint64)
    inp = inp.reshape(pr.shape[0], -1, 4) if inp.size else np.zeros((pr.shape[0], 0, 4), np.uint64)     # a key without public inputs
    w = _weights(weights, pr.shape[0])
    wf = np.zeros(pr.shape[0], np.uint8)
    accept, rep = C.c_int(0), AggReport()
    ch = ctx.handle if ctx is not None else None
    fn = lib.fk_verify_aggregate_dev if ctx is not None else lib.fk_verify_aggregate
    rc = fn(ch, _vp(vkb), vkb.size, _vp(inp) if inp.size else None, inp.shape[1], _vp(pr) if pr.size else None, pr.shape[0],
            _vp(w) if w is not None and w.size else None, _vp(wf) if wf.size else None, C.byref(accept), C.byref(rep))
    _check(rc, fn.__name__, lib.fk_last_error, ch)
    return bool(accept.value), wf.astype(bool), rep


def verify_batch_aggregated(ctx, vk_borsh, inputs, proofs):
    """The verdicts of `api.verify_batch(ctx, ...)`, at the price of one aggregated equation when every proof is good.  The fallback
    rule: an aggregate that does not accept hands the well-formed proofs to the per-proof kernel; a proof that is not well-formed is
    False.  ctx None: the host form (fk_verify_aggregate, then `api.verify` proof by proof) -- slow, for machines without a GPU."""
    pr = np.ascontiguousarray(proofs, np.uint8).reshape(-1, FK_PROOF_BYTES)
    inp = np.ascontiguousarray(inputs, np.uint64)
    inp = inp.reshape(pr.shape[0], -1, 4) if inp.size else np.zeros((pr.shape[0], 0, 4), np.uint64)
    accept, wf, _ = verify_aggregate(ctx, vk_borsh, inp, pr)
    if accept:
        return np.ones(pr.shape[0], bool)
    out = np.zeros(pr.shape[0], bool)
    idx = np.flatnonzero(wf)
    if idx.size:
        if ctx is not None:
            out[idx] = api.verify_batch(ctx, vk_borsh, inp[idx], pr[idx])
        else:
            out[idx] = [api.verify(vk_borsh, inp[i], pr[i].tobytes()) for i in idx]
    return out
