"""
Key ceremony, phase 1 (include/fawkes_hip_powers.h, csrc/powers.hip): contribute to a powers-of-tau
transcript on the device, validate the points of one, and check that one transcript is another with exactly one contribution applied.

`contribute` multiplies tau, alpha and beta of a transcript by secrets x, y, z: element i of every array times its own scalar (x^i, y x^i,
z x^i), one point per lane of `scale_powers`' kernel; it returns the new transcript and the public part of the contribution ([x] G2, [y] G2,
[z] G2).  `new_powers(m)` is the transcript of tau = alpha = beta = 1, so `contribute(ctx, new_powers(m), tau, alpha, beta)` makes one from
known secrets.  `validate_points` sorts points into infinity / out of range / off the curve / outside the subgroup / good;
`check_update` decides -- without any secret -- whether `after` is `before` with the contribution `pub` applied: the points of `after`,
`ceremony_init.check_powers` on `after`, and three pairing equations that bind it to `before`.  `ceremony_init.initial_key` takes the
transcript from there.  `contribute_host`, `check_update_host` and the entries with `ctx=None` are the plain host references (no GPU).

The weights of the check must not be predictable by whoever made `after`: leave `seed=None` (the library draws 32 bytes from getrandom(2)
per call) outside tests.

Not here: BGM17's proofs of knowledge and transcript hash, the .ptau format or any other file format, multi-GPU.  The C prototypes of
these entry points live in this module's own table (the table of _abi.py mirrors fawkes_hip.h and nothing else).
"""
import ctypes as C

import numpy as np

from . import api
from .api import _fr, _vp
from .ceremony import _ck, _seed
from .ceremony_init import PowersOfTau, PowersReport, PowersReportStruct, POWERS

I, U64, P = C.c_int, C.c_uint64, C.c_void_p

ARRAYS = ('tau_g1', 'tau_g2', 'alpha_tau_g1', 'beta_tau_g1', 'beta_g2')


class PowersOutStruct(C.Structure):
    """fk_powers_out"""
    _fields_ = [(n, C.c_void_p) for n in ARRAYS]


class PowersPublicStruct(C.Structure):
    """fk_powers_public"""
    _fields_ = [(n, C.c_uint8 * 128) for n in ('x_g2', 'y_g2', 'z_g2')]


class PointsReportStruct(C.Structure):
    """fk_points_report"""
    _fields_ = [(n, C.c_uint64) for n in ('infinity', 'range', 'curve', 'subgroup', 'first_bad')]


class PowersUpdateReportStruct(C.Structure):
    """fk_powers_update_report"""
    _fields_ = [(n, C.c_int32) for n in ('accept', 'shape_ok', 'points_ok', 'step_tau', 'step_alpha', 'step_beta', 'changed', 'reserved')] + \
               [(n, PointsReportStruct) for n in ARRAYS] + [('after', PowersReportStruct)]


OUT, PUBLIC, POINTS, UPDATE = C.POINTER(PowersOutStruct), C.POINTER(PowersPublicStruct), C.POINTER(PointsReportStruct), C.POINTER(PowersUpdateReportStruct)

# one prototype per function of include/fawkes_hip_powers.h: name -> (restype, argtypes)
PROTOTYPES = {
    'fk_g1_scale_powers_dev': (I, (P, P, U64, U64, P, P, P)),
    'fk_g2_scale_powers_dev': (I, (P, P, U64, U64, P, P, P)),
    'fk_g1_scale_powers': (I, (P, P, U64, U64, P, P, P)),
    'fk_g2_scale_powers': (I, (P, P, U64, U64, P, P, P)),
    'fk_powers_new': (I, (U64, OUT)),
    'fk_powers_contribute': (I, (P, POWERS, P, P, P, OUT, PUBLIC)),
    'fk_powers_contribute_host': (I, (POWERS, P, P, P, OUT, PUBLIC)),
    'fk_points_validate': (I, (P, P, U64, I, POINTS)),
    'fk_points_validate_dev': (I, (P, P, U64, I, P)),
    'fk_powers_update_check': (I, (P, POWERS, POWERS, PUBLIC, U64, P, UPDATE)),
    'fk_powers_update_check_host': (I, (POWERS, POWERS, PUBLIC, U64, P, UPDATE)),
}

FLAGS = ('shape_ok', 'points_ok', 'step_tau', 'step_alpha', 'step_beta')
NO_BAD_POINT = (1 << 64) - 1

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


class PowersPublic:
    """The public part of a contribution: x_g2, y_g2, z_g2 = [x] G2, [y] G2, [z] G2 as (128,) uint8 raw affine points."""

    def __init__(self, x_g2, y_g2, z_g2):
        self.x_g2, self.y_g2, self.z_g2 = (np.ascontiguousarray(p, np.uint8).reshape(128).copy() for p in (x_g2, y_g2, z_g2))

    def struct(self):
        st = PowersPublicStruct()
        for n in ('x_g2', 'y_g2', 'z_g2'):
            C.memmove(getattr(st, n), _vp(getattr(self, n)), 128)
        return st

    def replace(self, **over):
        a = dict(x_g2=self.x_g2, y_g2=self.y_g2, z_g2=self.z_g2)
        a.update(over)
        return PowersPublic(**a)


class PointsReport:
    """fk_points_report: the points per class (`infinity`, `range`, `curve`, `subgroup`) and `first_bad`, the lowest index in any of the
    four classes (None if there is none)."""

    def __init__(self, st):
        self.infinity, self.range, self.curve, self.subgroup = int(st.infinity), int(st.range), int(st.curve), int(st.subgroup)
        self.first_bad = None if int(st.first_bad) == NO_BAD_POINT else int(st.first_bad)

    @property
    def ok(self):
        return not (self.infinity or self.range or self.curve or self.subgroup)

    def counts(self):
        return dict(infinity=self.infinity, range=self.range, curve=self.curve, subgroup=self.subgroup)

    def __eq__(self, other):
        return isinstance(other, PointsReport) and self.counts() == other.counts() and self.first_bad == other.first_bad

    def __repr__(self):
        return 'PointsReport(%r, first_bad=%r)' % (self.counts(), self.first_bad)


class PowersUpdateReport:
    """What an update check found: the five flags of fk_powers_update_report as bools (`flags()`), `changed` (informational), the
    PointsReport of every array of `after` (`points`, by array name), `after` -- the PowersReport of the transcript check on `after` --
    and `accept`: the five flags and `after.accept`."""

    def __init__(self, st):
        for n in FLAGS + ('changed',):
            setattr(self, n, bool(getattr(st, n)))
        self.accept = bool(st.accept)
        self.points = {n: PointsReport(getattr(st, n)) for n in ARRAYS}
        self.after = PowersReport(st.after)

    def flags(self):
        return {n: getattr(self, n) for n in FLAGS}


def _out_for(counts):
    """(PowersOfTau of zeros with these counts, fk_powers_out over its arrays)"""
    n1, n2, na, nb = counts
    pw = PowersOfTau(np.zeros((n1, 64), np.uint8), np.zeros((n2, 128), np.uint8), np.zeros((na, 64), np.uint8), np.zeros((nb, 64), np.uint8), np.zeros(128, np.uint8))
    st = PowersOutStruct()
    for n in ARRAYS:
        setattr(st, n, getattr(pw, n).ctypes.data)
    return pw, st


def new_powers(m):
    """fk_powers_new: the transcript of tau = alpha = beta = 1 for a domain of m (2m - 1 generators in tau_g1, m in the others); no GPU"""
    lib = _lib()
    m = int(m)
    if m < 1:
        raise ValueError('a domain holds at least one element')
    pw, st = _out_for((2 * m - 1, m, m, m))
    _ck(lib, None, lib.fk_powers_new(m, C.byref(st)), 'fk_powers_new')
    return pw


def _contribute(ctx, powers, x, y, z):
    lib = _lib()
    x, y, z = _fr(x, 1), _fr(y, 1), _fr(z, 1)
    d = powers.desc()
    pw, st = _out_for((d.n_tau_g1, d.n_tau_g2, d.n_alpha_g1, d.n_beta_g1))
    pub = PowersPublicStruct()
    if ctx is None:
        _ck(lib, None, lib.fk_powers_contribute_host(C.byref(d), _vp(x), _vp(y), _vp(z), C.byref(st), C.byref(pub)), 'fk_powers_contribute_host')
    else:
        _ck(lib, ctx, lib.fk_powers_contribute(ctx.handle, C.byref(d), _vp(x), _vp(y), _vp(z), C.byref(st), C.byref(pub)), 'fk_powers_contribute')
    return pw, PowersPublic(bytearray(pub.x_g2), bytearray(pub.y_g2), bytearray(pub.z_g2))


def contribute(ctx, powers, x, y, z):
    """fk_powers_contribute: (PowersOfTau, PowersPublic) -- `powers` with tau, alpha, beta multiplied by x, y, z (Montgomery limbs, nonzero),
    every array whole, through the kernel; `powers` is only read"""
    return _contribute(ctx, powers, x, y, z)


def contribute_host(powers, x, y, z):
    """fk_powers_contribute_host: the reference of `contribute`; no GPU, ~0.2 ms per G1 point and three times that per G2 point"""
    return _contribute(None, powers, x, y, z)


def _group(points):
    pts = np.ascontiguousarray(points, np.uint8)
    if pts.ndim != 2 or pts.shape[1] not in (64, 128):
        raise ValueError('points are (n, 64) rows of G1 or (n, 128) rows of G2')
    return pts, pts.shape[1] == 128


def scale_powers(ctx, points, x, c=None, first=0):
    """out[i] = [c x^(first + i)] points[i]: (n, 64) G1 or (n, 128) G2 rows, the group by the row width; x, c: Montgomery limbs (c None: 1).
    ctx None: the host reference, else the kernel."""
    lib = _lib()
    pts, g2 = _group(points)
    x, c = _fr(x, 1), _fr(api._fr_rows([1]) if c is None else c, 1)
    out = np.zeros_like(pts)
    name = 'fk_g2_scale_powers' if g2 else 'fk_g1_scale_powers'
    n = pts.shape[0]
    _ck(lib, ctx, getattr(lib, name)(ctx.handle if ctx is not None else None, _vp(pts) if n else None, n, first, _vp(x), _vp(c), _vp(out) if n else None), name)
    return out


def scale_powers_dev(ctx, d_in, n, x, c, first, d_out, g2=False):
    """fk_g1_scale_powers_dev / fk_g2_scale_powers_dev: device pointers, asynchronous on the library's stream; d_out may be d_in"""
    lib = _lib()
    x, c = _fr(x, 1), _fr(c, 1)
    name = 'fk_g2_scale_powers_dev' if g2 else 'fk_g1_scale_powers_dev'
    _ck(lib, ctx, getattr(lib, name)(ctx.handle, d_in, n, first, _vp(x), _vp(c), d_out), name)


def validate_points(ctx, points):
    """fk_points_validate over (n, 64) G1 or (n, 128) G2 rows: a PointsReport.  ctx None: the host reference, else the kernel."""
    lib = _lib()
    pts, g2 = _group(points)
    st = PointsReportStruct()
    n = pts.shape[0]
    _ck(lib, ctx, lib.fk_points_validate(ctx.handle if ctx is not None else None, _vp(pts) if n else None, n, 1 if g2 else 0, C.byref(st)), 'fk_points_validate')
    return PointsReport(st)


def validate_points_dev(ctx, d_points, n, g2, d_report):
    """fk_points_validate_dev: points and report (40 bytes, the layout of fk_points_report) in device memory, asynchronous"""
    lib = _lib()
    _ck(lib, ctx, lib.fk_points_validate_dev(ctx.handle, d_points, n, 1 if g2 else 0, d_report), 'fk_points_validate_dev')


def _check_update(ctx, before, after, pub, m, seed):
    lib = _lib()
    s = _seed(seed)
    db, da, p = before.desc(), after.desc(), pub.struct()
    st = PowersUpdateReportStruct()
    if ctx is None:
        _ck(lib, None, lib.fk_powers_update_check_host(C.byref(db), C.byref(da), C.byref(p), m, _vp(s), C.byref(st)), 'fk_powers_update_check_host')
    else:
        _ck(lib, ctx, lib.fk_powers_update_check(ctx.handle, C.byref(db), C.byref(da), C.byref(p), m, _vp(s), C.byref(st)), 'fk_powers_update_check')
    return PowersUpdateReport(st)


def check_update(ctx, before, after, pub, m, seed=None):
    """fk_powers_update_check over the prefixes a domain of m uses.  seed: None (drawn by the library) or 32 bytes -- tests only"""
    return _check_update(ctx, before, after, pub, m, seed)


def check_update_host(before, after, pub, m, seed):
    """fk_powers_update_check_host: the reference of `check_update` (plain loops, the same pairings); no GPU"""
    if seed is None:
        raise ValueError('the host reference takes its seed from the caller')
    return _check_update(None, before, after, pub, m, seed)
