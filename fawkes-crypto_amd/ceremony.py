"""
Key ceremony, phase 2 (include/fawkes_hip_ceremony.h, csrc/ceremony.hip): apply one delta contribution to a
proving key and check one, on the device.

A contribution multiplies delta by a secret x and divides the h and l queries by it; `contribute` does that to a resident key (a new key
comes back, the old one is untouched), `check` decides -- without x -- whether `after` is `before` with exactly that done to it: a random
linear combination of h and h' (l and l') under secret 128-bit weights, four multi-scalar multiplications and three pairing equations.
`contribute_image` / `check_image` go from one `Parameters` image to the next.  `contribute_host` / `check_host` are the plain host
references (no GPU) the device is compared with.

The weights must not be predictable by whoever made the contribution: leave `seed=None` (the library draws 32 bytes from getrandom(2) per
call) outside tests, and never use a seed that was known before `after` was published.  The check assumes the points are on their
curves and in the order-r subgroup: load with `FK_KEY_CHECKED` (check_image does).

Not here: BGM17's proof of knowledge of x and the transcript hash (the returned deltas and the report carry what they need), phase 1,
sharded keys.  The C prototypes of these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and
nothing else).
"""
import ctypes as C

import numpy as np

from . import api, params_io
from .api import _check, _fr, _vp
from ._abi import KEY

I, U32, Z, P = C.c_int, C.c_uint32, C.c_size_t, C.c_void_p


class ContributionReportStruct(C.Structure):
    """fk_contribution_report"""
    _fields_ = [(n, C.c_int32) for n in ('accept', 'shape_equal', 'fixed_equal', 'delta_nonzero', 'delta_pair', 'ratio_h', 'ratio_l', 'delta_changed')] + \
               [(n, C.c_uint8 * 64) for n in ('s_h', 's_h_after', 's_l', 's_l_after')] + [('seed', C.c_uint8 * 32)]


REPORT = C.POINTER(ContributionReportStruct)

# one prototype per function of include/fawkes_hip_ceremony.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_g1_scale_dev': (I, (P, P, Z, P, P)),
    'fk_g1_scale': (I, (P, P, Z, P, P)),
    'fk_key_contribute': (I, (P, P, P, U32, P)),
    'fk_key_contribute_host': (I, (KEY, P, P, P, P, P)),
    'fk_ceremony_weights': (I, (P, Z, P)),
    'fk_ceremony_weights_dev': (I, (P, P, Z, P)),
    'fk_key_contribution_check': (I, (P, P, P, P, REPORT)),
    'fk_key_contribution_check_host': (I, (KEY, KEY, P, REPORT)),
}

FLAGS = ('shape_equal', 'fixed_equal', 'delta_nonzero', 'delta_pair', 'ratio_h', 'ratio_l')

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


class ContributionReport:
    """What a check found: the six flags of fk_contribution_report as bools, `delta_changed` (informational: x = 1 is a valid
    contribution), the four sums as their 64 raw bytes and the seed the weights came from (the same check with this seed reproduces the
    report).  check_image adds `header_equal` (gate header and const tracker) and `vk_equal` (gamma_g2, ic); they are None elsewhere.
    `accept`: everything that was checked holds."""

    def __init__(self, st, header_equal=None, vk_equal=None):
        for n in FLAGS + ('delta_changed',):
            setattr(self, n, bool(getattr(st, n)))
        self.key_accept = bool(st.accept)
        self.s_h, self.s_h_after, self.s_l, self.s_l_after = bytes(st.s_h), bytes(st.s_h_after), bytes(st.s_l), bytes(st.s_l_after)
        self.seed = bytes(st.seed)
        self.header_equal, self.vk_equal = header_equal, vk_equal

    @property
    def accept(self):
        return self.key_accept and self.header_equal is not False and self.vk_equal is not False

    def flags(self):
        return {n: getattr(self, n) for n in FLAGS}


def _seed(seed):
    if seed is None:
        return None
    s = np.frombuffer(bytes(seed), np.uint8)
    if s.size != 32:
        raise ValueError('a seed is 32 bytes')
    return s


def _ck(lib, ctx, rc, name):
    _check(rc, name, lib.fk_last_error, ctx.handle if ctx is not None else None)


def scale_g1(ctx, points, k):
    """k * P for every row of points ((n, 64) uint8 raw affine, zeros = infinity); k: Montgomery limbs.  ctx None: the host reference
    (fk_g1_scale without a context), else the kernel."""
    lib = _lib()
    pts = np.ascontiguousarray(points, np.uint8).reshape(-1, 64)
    k = _fr(k, 1)
    out = np.zeros_like(pts)
    _ck(lib, ctx, lib.fk_g1_scale(ctx.handle if ctx is not None else None, _vp(pts) if pts.size else None, pts.shape[0], _vp(k), _vp(out) if pts.size else None), 'fk_g1_scale')
    return out


def scale_g1_dev(ctx, d_in, n, k, d_out):
    """fk_g1_scale_dev: device pointers, asynchronous on the library's stream; d_out may be d_in"""
    lib = _lib()
    k = _fr(k, 1)
    _ck(lib, ctx, lib.fk_g1_scale_dev(ctx.handle, d_in, n, _vp(k), d_out), 'fk_g1_scale_dev')


def weights(seed, n, ctx=None):
    """the n weights of a check under `seed` (32 bytes) as (n, 4) uint64 Montgomery limbs; ctx: generated on the device and downloaded"""
    lib = _lib()
    s = _seed(seed)
    out = np.zeros((n, 4), np.uint64)
    if ctx is None:
        _ck(lib, None, lib.fk_ceremony_weights(_vp(s), n, _vp(out) if n else None), 'fk_ceremony_weights')
        return out
    d = ctx.dev_alloc(max(out.nbytes, 32))
    try:
        _ck(lib, ctx, lib.fk_ceremony_weights_dev(ctx.handle, _vp(s), n, d), 'fk_ceremony_weights_dev')
        ctx.sync()
        return ctx.download(d, out.nbytes, np.uint64).reshape(n, 4) if n else out
    finally:
        ctx.dev_free(d)


def contribute(ctx, key, x=None, levels=False):
    """fk_key_contribute: a new resident key with delta times x (Montgomery limbs; None: drawn with api.sample_fr and forgotten) and h, l
    divided by it; `key` is untouched.  levels: derive the fixed-base levels now.  Returns (DeviceKey, dict(delta_g1, delta_g2)): the
    two points a verifying key needs replaced."""
    lib = _lib()
    x = _fr(api.sample_fr() if x is None else x, 1)
    h = C.c_void_p()
    _ck(lib, ctx, lib.fk_key_contribute(ctx.handle, key.handle, _vp(x), 0 if levels else api.FK_KEY_NO_LEVELS, C.byref(h)), 'fk_key_contribute')
    out = api.DeviceKey(ctx, h)
    vk = out.vk()
    return out, dict(delta_g1=vk['delta_g1'], delta_g2=vk['delta_g2'])


def check(ctx, before, after, seed=None):
    """fk_key_contribution_check over two resident keys.  seed: None (drawn by the library) or 32 bytes -- tests only"""
    lib = _lib()
    s = _seed(seed)
    st = ContributionReportStruct()
    _ck(lib, ctx, lib.fk_key_contribution_check(ctx.handle, before.handle, after.handle, _vp(s), C.byref(st)), 'fk_key_contribution_check')
    return ContributionReport(st)


def contribute_host(params, x):
    """fk_key_contribute_host: the contributed key as a new api.Parameters (same constraint system); no GPU, ~0.17 ms per point"""
    lib = _lib()
    x = _fr(x, 1)
    d = params.desc()
    h, l = np.zeros_like(params.h), np.zeros_like(params.l)
    d1, d2 = np.zeros(64, np.uint8), np.zeros(128, np.uint8)
    _ck(lib, None, lib.fk_key_contribute_host(C.byref(d), _vp(x), _vp(h) if h.size else None, _vp(l) if l.size else None, _vp(d1), _vp(d2)), 'fk_key_contribute_host')
    arrays = dict(m=params.m, num_input=params.num_input, num_aux=params.num_aux, h=h, l=l, a=params.a, b_g1=params.b_g1, b_g2=params.b_g2)
    arrays.update(params.vk)
    arrays.update(delta_g1=d1, delta_g2=d2)
    return api.Parameters(arrays, params.r1cs)


def check_host(params_before, params_after, seed):
    """fk_key_contribution_check_host over two api.Parameters: the reference of `check` (naive sums, the same pairings); no GPU"""
    lib = _lib()
    s = _seed(seed)
    db, da = params_before.desc(), params_after.desc()
    st = ContributionReportStruct()
    _ck(lib, None, lib.fk_key_contribution_check_host(C.byref(db), C.byref(da), _vp(s), C.byref(st)), 'fk_key_contribution_check_host')
    return ContributionReport(st)


_IMAGE_FLAGS = api.FK_KEY_CHECKED | api.FK_KEY_NO_LEVELS


def _split_image(image):
    """(bytes in front of the bellman part: gate header, blob, const tracker; the bellman part) as views into the image"""
    view = api._bytes_view(image)
    hdr = params_io.read_parameters(view)
    n = len(hdr['bellman'])
    return view[:view.size - n], view[view.size - n:]


def contribute_image(ctx, image, x=None):
    """One contribution from a `Parameters` image to the next: the key is read with the point checks of Parameters::read(checked)
    (fk_key_load_bellman, FK_KEY_CHECKED), contributed to on the device and written back (fk_key_write_bellman); gates, const tracker,
    gamma_g2 and ic carry over unchanged.  Returns the new image as bytes."""
    head, bellman = _split_image(image)
    key, gamma_g2, ic = ctx.load_key_bellman(bellman, flags=_IMAGE_FLAGS)
    try:
        new, _ = contribute(ctx, key, x)
        try:
            out = ctx.write_key_bellman(new, dict(gamma_g2=gamma_g2, ic=ic))
        finally:
            new.free()
    finally:
        key.free()
    return head.tobytes() + out.tobytes()


def check_image(ctx, image_before, image_after, seed=None):
    """`check` over two `Parameters` images, both loaded with FK_KEY_CHECKED (a malformed image raises the loader's FkError); also
    compares the gate header with the const tracker (`header_equal`) and gamma_g2 and ic (`vk_equal`) byte for byte."""
    hb, bb = _split_image(image_before)
    ha, ba = _split_image(image_after)
    kb, gamma_b, ic_b = ctx.load_key_bellman(bb, flags=_IMAGE_FLAGS)
    try:
        ka, gamma_a, ic_a = ctx.load_key_bellman(ba, flags=_IMAGE_FLAGS)
        try:
            rep = check(ctx, kb, ka, seed)
        finally:
            ka.free()
    finally:
        kb.free()
    rep.header_equal = hb.tobytes() == ha.tobytes()
    rep.vk_equal = gamma_b.tobytes() == gamma_a.tobytes() and ic_b.tobytes() == ic_a.tobytes()
    return rep
