"""Support shared by test_gpu_field_ops.py, test_gpu_point_ops.py and the tower tests (_tower_cases.py): the ctypes binding of the
test-only library libfawkes_fieldtest.so (csrc/fieldtest.hip, csrc/fieldtest_tower.hip), its type / operation / mode tables, the limb
encoding and the generators of edge and structured limb images.

Values are Python integers throughout: an element of a base field is an int, an element of an Fq2 type is a pair (c0, c1).  What
goes to the device and comes back is the Montgomery limb image itself (8 x u32 little endian = 32 bytes little endian), not a
value converted on the way: the tests choose the limbs.
"""
import ctypes as C
import functools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, 'fawkes-crypto_amd', 'libfawkes_fieldtest.so')

P_FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
P_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT_R = 1 << 256


class Type:
    def __init__(self, name, tid, p, lazy=False, fq2=False, points=True):
        self.name, self.id, self.p, self.lazy, self.fq2, self.points = name, tid, p, lazy, fq2, points
        self.q = 2 * p if lazy else p           # operands and results live in [0, q)
        self.w = 2 if fq2 else 1                # base-field values per element
        self.rinv = pow(MONT_R, -1, p)

    def __repr__(self):
        return self.name


# ids as in csrc/fieldtest.hip
TYPES = [Type('Fq', 0, P_FQ), Type('FqL', 1, P_FQ, lazy=True), Type('FqC', 2, P_FQ),
         Type('Fr', 3, P_FR, points=False), Type('FrL', 4, P_FR, lazy=True, points=False),
         Type('Fq2', 5, P_FQ, fq2=True), Type('Fq2L', 6, P_FQ, lazy=True, fq2=True), Type('Fq2C', 7, P_FQ, fq2=True)]
TYPE = {t.name: t for t in TYPES}
OP_NAMES = ['add', 'sub', 'dbl', 'neg', 'add2', 'sub2', 'addsub2', 'mul', 'sqr', 'mul2', 'sqr2', 'mulsub', 'dot4',
            'is_zero', 'eq', 'canon', 'from_mont', 'to_mont',
            'p_add_mixed', 'p_add_mixed_nz', 'p_add', 'p_dbl', 'p_dbl_affine', 'p_neg_if', 'p_to_affine',
            'inv', 'pow', 'pow_u64', 'from_u64', 'p_mul_scalar', 'p_mul_affine_bits']      # ids stay: new operations go to the end
OP = {n: i for i, n in enumerate(OP_NAMES)}
MODE = {'straight': 0, 'divergent': 1, 'aliased': 2}
# ids as in csrc/fieldtest_tower.hip
TOWER_OPS = ['f6_mul', 'f6_mul_by_01', 'f6_mul_by_fq2', 'f6_mul_v', 'f6_mul_xi', 'f6_inv', 'f6_add', 'f6_sub', 'f6_neg',
             'f12_mul', 'f12_sqr_complex', 'f12_mul_by_line', 'f12_conj', 'f12_inv', 'f12_is_one', 'f12_pow',
             'miller_loop', 'miller_loop_proj', 'final_exp']
TOWER_OP = {n: i for i, n in enumerate(TOWER_OPS)}
WHERE = {'device': 0, 'host': 1}


class FieldTestLib:
    """One per test module.  The first non-zero return code is kept: every later run() of the module fails at once, without a
    launch (a failed launch is not retried, and nothing is started on a device that has just reported an error)."""

    def __init__(self):
        self._lib = None
        self.failed = None
        self.cases_run = {}                      # (type, op, mode) -> cases, for the summary the module prints

    def lib(self):
        if self._lib is None:
            lib = C.CDLL(LIB_PATH)               # no fallback: a missing library is an error (build() makes it)
            lib.ft_last_error.restype = C.c_char_p
            lib.ft_run.restype = C.c_int
            lib.ft_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
            lib.ft_supported.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            lib.ft_tower_shape.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            lib.ft_tower_run.restype = C.c_int
            lib.ft_tower_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
            self._lib = lib
        return self._lib

    def shape(self, t, op, mode):
        """(operands, results) in elements per case, or None if the library has no such kernel"""
        ni, no = C.c_int(0), C.c_int(0)
        if not self.lib().ft_supported(t.id, OP[op], MODE[mode], C.byref(ni), C.byref(no)):
            return None
        return ni.value, no.value

    def alt(self, op):
        a = self.lib().ft_alt_op(OP[op])
        return None if a < 0 else OP_NAMES[a]

    def run(self, t, op, mode, cases):
        """cases: a list of tuples of elements -> the list of result tuples"""
        if self.failed:
            pytest.fail('not launched: an earlier call of this module failed (%s)' % self.failed)
        ni, no = self.shape(t, op, mode)
        n = len(cases)
        assert n and all(len(c) == ni for c in cases)
        if t.fq2:
            data = b''.join(v.to_bytes(32, 'little') for c in cases for e in c for v in e)
        else:
            data = b''.join(e.to_bytes(32, 'little') for c in cases for e in c)
        assert len(data) == n * ni * t.w * 32
        out = C.create_string_buffer(n * no * t.w * 32)
        rc = self.lib().ft_run(t.id, OP[op], MODE[mode], data, ni, out, no, n)
        if rc != 0:
            self.failed = 'ft_run(%s, %s, %s) returned %d: %s' % (t, op, mode, rc, (self.lib().ft_last_error() or b'').decode())
            pytest.fail(self.failed)
        key = (t.name, op, mode)
        self.cases_run[key] = self.cases_run.get(key, 0) + n
        mv = memoryview(out.raw)
        vals = [int.from_bytes(mv[i:i + 32], 'little') for i in range(0, len(mv), 32)]
        if t.fq2:
            vals = list(zip(vals[0::2], vals[1::2]))
        return [tuple(vals[i * no:(i + 1) * no]) for i in range(n)]


    def tower_shape(self, op_id):
        """(words in, words out) of one case of a tower operation, or None"""
        wi, wo = C.c_int(0), C.c_int(0)
        if not self.lib().ft_tower_shape(op_id, C.byref(wi), C.byref(wo)):
            return None
        return wi.value, wo.value

    def run_tower(self, op, where, cases):
        """cases: a list of byte strings, each the words of one case -> the list of the cases' result bytes"""
        if self.failed:
            pytest.fail('not launched: an earlier call of this module failed (%s)' % self.failed)
        wi, wo = self.tower_shape(TOWER_OP[op])
        n = len(cases)
        assert n and all(len(c) == 4 * wi for c in cases), (op, wi, [len(c) for c in cases][:4])
        out = C.create_string_buffer(n * wo * 4)
        rc = self.lib().ft_tower_run(TOWER_OP[op], WHERE[where], b''.join(cases), wi, out, wo, n)
        if rc != 0:
            self.failed = 'ft_tower_run(%s, %s) returned %d: %s' % (op, where, rc, (self.lib().ft_last_error() or b'').decode())
            pytest.fail(self.failed)
        key = (where, op, 'tower')
        self.cases_run[key] = self.cases_run.get(key, 0) + n
        raw = out.raw
        return [raw[i * wo * 4:(i + 1) * wo * 4] for i in range(n)]


# ------------------------------------------------------------------------------------------------ limb images worth trying
LIMB_PICKS = (0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff)


@functools.lru_cache(maxsize=None)
def edge_list(p, lazy):
    q = 2 * p if lazy else p
    r = MONT_R % p
    vals = [0, 1, 2, p - 1, p, p + 1, 2 * p - 1, q - 1, r, r * r % p]
    if lazy:
        vals += [r + p, r * r % p + p]
    for k in (31, 32, 33, 63, 64, 224, 253):
        vals += [1 << k, (1 << k) - 1]
    vals += [0xffffffff << (32 * i) for i in range(8)]
    vals.append(sum(0x80000000 << (32 * i) for i in range(8)))
    qtop, out = q >> 224, []
    for v in vals:
        if v >= q:                  # clipped: the low seven limbs stay, the top limb comes under q's
            v = (v & ((1 << 224) - 1)) | (min(v >> 224, qtop - 1) << 224)
        assert 0 <= v < q
        if v not in out:
            out.append(v)
    return tuple(out)


def structured(rnd, q):
    qtop = q >> 224
    v = 0
    for i in range(7):
        k = rnd.randrange(7)
        v |= (LIMB_PICKS[k] if k < 6 else rnd.getrandbits(32)) << (32 * i)
    tops = [x for x in LIMB_PICKS if x < qtop]
    k = rnd.randrange(len(tops) + 1)
    return v | ((tops[k] if k < len(tops) else rnd.randrange(qtop)) << 224)


def first_limb_odd(t, element):
    """the predicate of divergent mode: bit 0 of limb 0 of the case's first operand"""
    return bool((element[0] if t.fq2 else element) & 1)


def check_element(t, got, want, exact=False):
    """None if `got` (limb image) is a valid result for the exact value `want`, else a description.
    Canonical types (and results stated to be exact): got == want mod p, bit for bit.  Lazy types: got < 2p and got = want mod p."""
    gs, ws = (got, want) if t.fq2 else ((got,), (want,))
    for g, w in zip(gs, ws):
        if exact or not t.lazy:
            if g != w % t.p:
                return 'not the canonical value'
        elif g >= t.q:
            return 'not below 2p'
        elif g % t.p != w % t.p:
            return 'not congruent'
    return None


def hexel(t, e):
    return '(%s)' % ', '.join('%#x' % v for v in e) if t.fq2 else '%#x' % e
