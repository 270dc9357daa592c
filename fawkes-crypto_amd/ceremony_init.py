"""
Key ceremony, the start of phase 2 (include/fawkes_hip_ceremony_init.h, csrc/ceremony_init.hip): the initial
proving key of a circuit from a powers-of-tau transcript, and the transcript's check, on the device.

`initial_key` derives, from the group elements [tau^i] G1, [tau^i] G2, [alpha tau^i] G1, [beta tau^i] G1 and [beta] G2 alone, the key that
`Context.setup` gives for the same tau, alpha, beta and gamma = delta = 1: four inverse transforms over group elements (`g1_ntt`, `g2_ntt`
are those transforms on their own) and one linear combination of points per variable.  `ceremony.contribute` takes the key from there.
`check_powers` says whether the prefixes of the transcript a domain of m uses are consistent (geometric sequences with one ratio, tied
to tau_g2[1] and beta_g2): a key derived from an inconsistent transcript is silently worthless.  `initial_key_host`, `check_powers_host`
and the transforms with `ctx=None` are the plain host references (no GPU) the device is compared with.  `initial_image` replaces the key
of a `Parameters` image by the initial key of its own gates.

The weights of the check must not be predictable by whoever made the transcript: leave `seed=None` (the library draws 32 bytes from
getrandom(2) per call) outside tests.  Check and derivation assume the points are on their curves and in the order-r subgroup.

Not here: tiled systems, sharded and multi-GPU keys, BGM17's transcript hash and proofs of knowledge, the file format of any phase-1
tool.  The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
"""
import ctypes as C

import numpy as np

from . import api, params_io
from .api import _vp
from ._abi import CS
from .ceremony import _ck, _seed

I, U32, U64, P = C.c_int, C.c_uint32, C.c_uint64, C.c_void_p


class PowersDesc(C.Structure):
    """fk_powers_desc"""
    _fields_ = [(n, C.c_uint64) for n in ('n_tau_g1', 'n_tau_g2', 'n_alpha_g1', 'n_beta_g1')] + \
               [(n, C.c_void_p) for n in ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1', 'beta_g2')]


class PowersReportStruct(C.Structure):
    """fk_powers_report"""
    _fields_ = [(n, C.c_int32) for n in ('accept', 'gen_ok', 'tau_pair', 'ratio_tau_g1', 'ratio_tau_g2', 'ratio_alpha', 'ratio_beta', 'beta_pair')] + \
               [(n, C.c_uint8 * 64) for n in ('s_tau_g1', 's_tau_g1_next', 's_alpha', 's_alpha_next', 's_beta', 's_beta_next')] + \
               [(n, C.c_uint8 * 128) for n in ('s_tau_g2', 's_tau_g2_next')] + [('seed', C.c_uint8 * 32)]


POWERS, REPORT = C.POINTER(PowersDesc), C.POINTER(PowersReportStruct)

# one prototype per function of include/fawkes_hip_ceremony_init.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_g1_ntt_dev': (I, (P, P, U32, I)),
    'fk_g2_ntt_dev': (I, (P, P, U32, I)),
    'fk_g1_ntt': (I, (P, P, U32, I, P)),
    'fk_g2_ntt': (I, (P, P, U32, I, P)),
    'fk_key_from_powers': (I, (P, POWERS, CS, U32, P, P, P)),
    'fk_key_from_powers_host': (I, (POWERS, CS, P, P, P, P, P, P, P, P)),
    'fk_powers_check': (I, (P, POWERS, U64, P, REPORT)),
    'fk_powers_check_host': (I, (POWERS, U64, P, REPORT)),
}

FLAGS = ('gen_ok', 'tau_pair', 'ratio_tau_g1', 'ratio_tau_g2', 'ratio_alpha', 'ratio_beta', 'beta_pair')
SUMS = ('s_tau_g1', 's_tau_g1_next', 's_alpha', 's_alpha_next', 's_beta', 's_beta_next', 's_tau_g2', 's_tau_g2_next')

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


class PowersOfTau:
    """A powers-of-tau transcript in memory: tau_g1 (n, 64), tau_g2 (n, 128), alpha_tau_g1 (n, 64), beta_tau_g1 (n, 64) uint8 rows of raw
    affine Montgomery LE points (zeros = infinity) and beta_g2 (128).  A circuit with domain m needs 2m - 1 rows of tau_g1 and m of the
    others; longer arrays are used by their prefixes."""

    def __init__(self, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2):
        self.tau_g1 = np.ascontiguousarray(tau_g1, np.uint8).reshape(-1, 64)
        self.tau_g2 = np.ascontiguousarray(tau_g2, np.uint8).reshape(-1, 128)
        self.alpha_tau_g1 = np.ascontiguousarray(alpha_tau_g1, np.uint8).reshape(-1, 64)
        self.beta_tau_g1 = np.ascontiguousarray(beta_tau_g1, np.uint8).reshape(-1, 64)
        self.beta_g2 = np.ascontiguousarray(beta_g2, np.uint8).reshape(128)

    def desc(self):
        """fk_powers_desc over this object's arrays (which must outlive it)"""
        d = PowersDesc()
        d.n_tau_g1, d.n_tau_g2, d.n_alpha_g1, d.n_beta_g1 = self.tau_g1.shape[0], self.tau_g2.shape[0], self.alpha_tau_g1.shape[0], self.beta_tau_g1.shape[0]
        for n in ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1', 'beta_g2'):
            setattr(d, n, getattr(self, n).ctypes.data)
        return d

    def prefix(self, m):
        """the transcript cut to what a domain of m needs (views, no copy)"""
        return PowersOfTau(self.tau_g1[:2 * m - 1], self.tau_g2[:m], self.alpha_tau_g1[:m], self.beta_tau_g1[:m], self.beta_g2)

    def replace(self, **over):
        """a copy with some arrays replaced"""
        a = {n: getattr(self, n) for n in ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1', 'beta_g2')}
        a.update(over)
        return PowersOfTau(**a)


class PowersReport:
    """What a transcript check found: the seven flags of fk_powers_report as bools, `accept` (all of them), the eight sums as raw bytes
    and the seed the weights came from (the same check with this seed reproduces the report)."""

    def __init__(self, st):
        for n in FLAGS:
            setattr(self, n, bool(getattr(st, n)))
        self.accept = bool(st.accept)
        for n in SUMS:
            setattr(self, n, bytes(getattr(st, n)))
        self.seed = bytes(st.seed)

    def flags(self):
        return {n: getattr(self, n) for n in FLAGS}

    def sums(self):
        return {n: getattr(self, n) for n in SUMS}


def _ntt(name, width, ctx, points, inverse):
    lib = _lib()
    pts = np.ascontiguousarray(points, np.uint8).reshape(-1, width)
    n = pts.shape[0]
    if n < 1 or n & (n - 1):
        raise ValueError('a transform takes 2^k points')
    out = np.zeros_like(pts)
    _ck(lib, ctx, getattr(lib, name)(ctx.handle if ctx is not None else None, _vp(pts), n.bit_length() - 1, 1 if inverse else 0, _vp(out)), name)
    return out


def g1_ntt(ctx, points, inverse=False):
    """fk_g1_ntt: out[k] = sum_j [omega^(jk)] points[j] over (2^k, 64) raw G1 points, fk_ntt's convention (the inverse includes 1/n).
    ctx None: the host reference, else the kernels."""
    return _ntt('fk_g1_ntt', 64, ctx, points, inverse)


def g2_ntt(ctx, points, inverse=False):
    """fk_g2_ntt: the same over (2^k, 128) raw G2 points"""
    return _ntt('fk_g2_ntt', 128, ctx, points, inverse)


def g1_ntt_dev(ctx, d_points, log_n, inverse=False):
    """fk_g1_ntt_dev: 2^log_n affine G1 points on the device, in place, asynchronous on the library's stream"""
    lib = _lib()
    _ck(lib, ctx, lib.fk_g1_ntt_dev(ctx.handle, d_points, log_n, 1 if inverse else 0), 'fk_g1_ntt_dev')


def g2_ntt_dev(ctx, d_points, log_n, inverse=False):
    """fk_g2_ntt_dev: the same for G2 points"""
    lib = _lib()
    _ck(lib, ctx, lib.fk_g2_ntt_dev(ctx.handle, d_points, log_n, 1 if inverse else 0), 'fk_g2_ntt_dev')


def initial_key_dev(ctx, powers, r1cs, levels=False):
    """fk_key_from_powers: (DeviceKey, vk dict) as Context.setup returns them -- vk = alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1,
    delta_g2 and ic (num_input, 64)"""
    lib = _lib()
    h = C.c_void_p()
    vk = np.zeros(6 * 128, np.uint8)
    ic = np.zeros((r1cs.num_input, 64), np.uint8)
    d = powers.desc()
    _ck(lib, ctx, lib.fk_key_from_powers(ctx.handle, C.byref(d), C.byref(r1cs.struct), 0 if levels else api.FK_KEY_NO_LEVELS, C.byref(h), _vp(vk),
                                         _vp(ic) if ic.size else None), 'fk_key_from_powers')
    return api.DeviceKey(ctx, h), api._vk_dict(vk, ic)


class InitialParameters(api.Parameters):
    """The `Parameters` of an initial key: `key` is the resident key (initial_key; None for initial_key_host), `vk_full` the verifying
    key's six points and `ic`."""
    key = None
    vk_full = None

    @property
    def ic(self):
        return self.vk_full['ic']


def initial_key(ctx, powers, r1cs, levels=False):
    """The circuit's initial key from the transcript, on the device: an api.Parameters (host copies of the arrays, `r1cs` attached) that
    also holds the resident key (`.key`, a DeviceKey: free it when done), the verifying key (`.vk_full`: six points and ic) and `.ic`.
    levels: derive the fixed-base levels now."""
    key, vk = initial_key_dev(ctx, powers, r1cs, levels)
    arrays = dict(key.counts())
    arrays.update({n: key.download(n) for n in ('h', 'l', 'a', 'b_g1', 'b_g2')})
    arrays.update({n: vk[n] for n in ('alpha_g1', 'beta_g1', 'beta_g2', 'delta_g1', 'delta_g2')})
    out = InitialParameters(arrays, r1cs)
    out.key, out.vk_full = key, vk
    return out


def initial_key_host(powers, r1cs):
    """fk_key_from_powers_host: the same Parameters by plain host loops (no GPU; domains up to 2^8 or so), `.key` is None"""
    lib = _lib()
    rows = r1cs.num_gates + r1cs.num_input
    m = 1
    while m < rows:
        m *= 2
    nv = r1cs.num_input + r1cs.num_aux
    h, l = np.zeros((max(m - 1, 0), 64), np.uint8), np.zeros((r1cs.num_aux, 64), np.uint8)
    a, b1, b2 = np.zeros((nv, 64), np.uint8), np.zeros((nv, 64), np.uint8), np.zeros((nv, 128), np.uint8)
    counts = np.zeros(2, np.uint64)
    vk, ic = np.zeros(6 * 128, np.uint8), np.zeros((r1cs.num_input, 64), np.uint8)
    d = powers.desc()

    def ptr(x):
        return _vp(x) if x.size else None
    _ck(lib, None, lib.fk_key_from_powers_host(C.byref(d), C.byref(r1cs.struct), ptr(h), ptr(l), ptr(a), ptr(b1), ptr(b2), _vp(counts), _vp(vk), ptr(ic)),
        'fk_key_from_powers_host')
    n_a, n_b = int(counts[0]), int(counts[1])
    vkd = api._vk_dict(vk, ic)
    arrays = dict(m=m, num_input=r1cs.num_input, num_aux=r1cs.num_aux, h=h, l=l, a=a[:n_a].copy(), b_g1=b1[:n_b].copy(), b_g2=b2[:n_b].copy())
    arrays.update({n: vkd[n] for n in ('alpha_g1', 'beta_g1', 'beta_g2', 'delta_g1', 'delta_g2')})
    out = InitialParameters(arrays, r1cs)
    out.vk_full = vkd
    return out


def initial_image(ctx, powers, image):
    """The `Parameters` image of the initial key of `image`'s own gates: the gate blob is decoded (api.Gates), the key derived on the device
    (fk_key_from_powers) and written behind the image's header (fk_key_write_bellman); gates and const tracker carry over unchanged, the key
    the image held is only used for its counts.  Returns the new image as bytes."""
    view = api._bytes_view(image)
    hdr = params_io.read_parameters(view)
    c = params_io.bellman_counts(hdr['bellman'])
    blob = hdr['gates_blob']
    raw = bytes(blob[:len(params_io.RAW_MAGIC)]) == params_io.RAW_MAGIC
    gates = api.Gates(blob[len(params_io.RAW_MAGIC):] if raw else blob, api.FK_GATES_RAW if raw else api.FK_GATES_BROTLI, hdr['num_gates'], c['num_input'], c['num_aux'], ctx=None)
    try:
        r1cs = gates.to_r1cs()
    finally:
        gates.free()
    key, vk = initial_key_dev(ctx, powers, r1cs)
    try:
        out = ctx.write_key_bellman(key, vk)
    finally:
        key.free()
    head = view[:view.size - len(hdr['bellman'])]
    return head.tobytes() + out.tobytes()


def check_powers(ctx, powers, m, seed=None):
    """fk_powers_check over the prefixes a domain of m uses.  seed: None (drawn by the library) or 32 bytes -- tests only"""
    lib = _lib()
    s = _seed(seed)
    st = PowersReportStruct()
    d = powers.desc()
    _ck(lib, ctx, lib.fk_powers_check(ctx.handle, C.byref(d), m, _vp(s), C.byref(st)), 'fk_powers_check')
    return PowersReport(st)


def check_powers_host(powers, m, seed):
    """fk_powers_check_host: the reference of `check_powers` (naive sums, the same pairings); no GPU"""
    lib = _lib()
    s = _seed(seed)
    st = PowersReportStruct()
    d = powers.desc()
    _ck(lib, None, lib.fk_powers_check_host(C.byref(d), m, _vp(s), C.byref(st)), 'fk_powers_check_host')
    return PowersReport(st)
