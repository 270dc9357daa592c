"""The front of a multiplication, stage by stage (csrc/msm.hip: digits, two-pass bucket sort, cap and oversized-bucket tables, size order),
run through the product's own host code by fk_msm_front_dump and compared EXACTLY with a reference held here in Python integers and numpy:
  * a scalar leaves Montgomery form (x * 2^-256 mod r, Python integers);
  * it is recoded over the plan's windows by the stated rule: window w has cb + (w < wide) bits; a raw value (window bits + carry) above
    2^(cw-1) becomes the negative digit 2^cw - raw with a carry into the next window.
Everything else (bucket totals, starts, the sorted runs, cap, oversized list, segment tasks, size order, addition count) is derived from
these reference digits.  The whole-multiplication tests (test_gpu_msm.py) see only the group element; a front that is wrong in a way the
back forgives -- a valid but unordered perm, a cap or an addition count that is off, a digit recoded by another rule -- shows only here.
The shapes step over the sort's boundaries: 8192 entries per first-pass sub-tile and second-pass tile, 16 384 per chunk, 1024 high bins,
1024 / 2048 low bins, the oversized-bucket limits and the 768-size knee of the size classes."""
import numpy as np
import pytest

from helpers import R, g1_bases

pytestmark = pytest.mark.gpu

RINV = pow(1 << 256, -1, R)


# ------------------------------------------------------------------------------------------ reference
def mont(ints):
    """canonical integers -> (n, 4) uint64 Montgomery limbs"""
    return np.frombuffer(b''.join(((v << 256) % R).to_bytes(32, 'little') for v in ints), np.uint64).reshape(-1, 4).copy()


def windows(p):
    """[(offset, bits)] of the plan's W windows"""
    out, o = [], 0
    for w in range(p['W']):
        cw = p['cb'] + (1 if w < p['wide'] else 0)
        out.append((o, cw))
        o += cw
    assert o == 255
    return out


def ref_digits(scalars, p):
    """(canonical ints, magnitude (W, n) int64, negative (W, n) bool) by the stated recoding rule"""
    n = scalars.shape[0]
    ints = [int.from_bytes(row.tobytes(), 'little') * RINV % R for row in scalars]
    bits = np.unpackbits(np.frombuffer(b''.join(v.to_bytes(32, 'little') for v in ints), np.uint8).reshape(n, 32), axis=1, bitorder='little')
    mag, neg = np.zeros((p['W'], n), np.int64), np.zeros((p['W'], n), bool)
    carry = np.zeros(n, np.int64)
    for w, (o, cw) in enumerate(windows(p)):
        raw = bits[:, o:o + cw].astype(np.int64) @ (np.int64(1) << np.arange(cw, dtype=np.int64)) + carry
        neg[w] = raw > (1 << (cw - 1))
        mag[w] = np.where(neg[w], (1 << cw) - raw, raw)
        carry = neg[w].astype(np.int64)
    assert not carry.any()          # r < 2^254: the top window never overflows
    return ints, mag, neg


def size_class(s, cap):
    """csrc/msm.hip size_class restated (s = min(size, cap)): one class per size below 768, 256 coarse classes above; larger sizes first"""
    s = s.astype(np.int64)
    span = cap - 768 if cap > 768 else 1
    return np.where(s < 768, 1023 - s, 255 - ((s - 768) * 255) // span)


def check_size_order(perm, lengths, cap, what):
    m = lengths.shape[0]
    assert perm.shape[0] == m and perm.max(initial=0) < m and (np.bincount(perm, minlength=m) == 1).all(), what + ': perm is not a permutation'
    key = np.minimum(lengths[perm].astype(np.int64), cap)
    up = np.nonzero(key[1:] > key[:-1])[0]              # the length may rise only between two members of one coarse class
    cls = size_class(key, cap)
    assert (key[up] >= 768).all() and (cls[up] == cls[up + 1]).all(), (what, up[:8], key[up][:8], key[up + 1][:8])
    assert (cls[1:] >= cls[:-1]).all(), what


def check_front(ctx, scalars, wb, merged, what):
    """runs the dump under `wb` forced window bits and compares every table; returns (plan, dyn)"""
    ctx.set_window_bits(wb)
    try:
        d = ctx.msm_front_dump(scalars, merged=merged)
    finally:
        ctx.set_window_bits(0)
    p, dyn = d['plan'], d['dyn']
    n, W, B = scalars.shape[0], p['W'], p['B']
    win = windows(p)
    ints, mag, neg = ref_digits(scalars, p)
    # ---- digits: word for word; and, independently of the rule's details, a signed-digit form of s with |d_w| <= 2^(cw-1)
    want = (mag | (neg.astype(np.int64) << 31)).astype(np.uint32)
    bad = np.argwhere(d['digits'] != want)
    assert bad.size == 0, (what, 'digits', bad[:4], [hex(int(d['digits'][w, i])) for w, i in bad[:4]], [hex(int(want[w, i])) for w, i in bad[:4]])
    got_mag, got_neg = (d['digits'] & 0x7fffffff).astype(np.int64), (d['digits'] >> 31).astype(bool)
    acc, part, base = np.zeros(n, object), np.zeros(n, np.int64), 0          # runs of windows spanning <= 60 bits are summed in int64
    for w, (o, cw) in enumerate(win):
        assert (got_mag[w] <= (1 << (cw - 1))).all(), (what, 'digit range', w)
        if o + cw - base > 60:
            acc, part, base = acc + part.astype(object) * (1 << base), np.zeros(n, np.int64), o
        part = part + (np.where(got_neg[w], -got_mag[w], got_mag[w]) << (o - base))
    acc = acc + part.astype(object) * (1 << base)
    assert list(acc) == ints, (what, 'digits do not sum to the scalar')
    # ---- sort: totals, starts, and every bucket's run as a multiset
    totals = np.stack([np.bincount(mag[w][mag[w] > 0] - 1, minlength=B) for w in range(W)]).astype(np.int64)
    starts = np.cumsum(totals, axis=1) - totals
    assert np.array_equal(d['totals'], totals), (what, 'totals', np.argwhere(d['totals'] != totals)[:4])
    assert np.array_equal(d['starts'], starts), (what, 'starts', np.argwhere(d['starts'] != starts)[:4])
    idx = np.arange(n, dtype=np.int64)
    for w in range(W):
        nz = mag[w] > 0
        want_keys = np.sort(((mag[w][nz] - 1) << 32) | idx[nz] | (neg[w][nz].astype(np.int64) << 31))
        cnt = int(totals[w].sum())
        got_keys = np.sort((np.repeat(np.arange(B, dtype=np.int64), totals[w]) << 32) | d['sorted'][w, :cnt].astype(np.int64))
        assert np.array_equal(got_keys, want_keys), (what, 'sorted runs of window', w, np.nonzero(got_keys != want_keys)[0][:4])
    # ---- cap (msm_cap_kernel's rule: doubled until at most `many` buckets stay above it, or it reaches 2^20) and the oversized list
    WB = W * B
    many = min(max(2048, WB // 8192), p['over_max'] - 64)
    k = 0
    while k < 15 and int((totals > (p['cap'] << k)).sum()) > many and (p['cap'] << k) < (1 << 20):
        k += 1
    cap = min(p['cap'] << k, 1 << 30)
    assert dyn['cap'] == cap, (what, 'cap', dyn['cap'], p['cap'], k)
    flat = totals.reshape(-1)
    over = np.nonzero(flat > cap)[0]
    assert dyn['n_over'] == over.size and dyn['error'] == 0, (what, dyn, over.size)
    # ---- segment tasks and fold groups
    seg, tasks, obs = dyn['seg'], d['tasks'].astype(np.int64), d['obs'].astype(np.int64)
    assert p['seg_min'] <= seg <= p['seg_max'] and seg % 64 == 0, (what, seg)
    # all oversized entries spread over about 2048 waves (two per SIMD), in multiples of 64 entries, inside [SEG_MIN, SEG_MAX]
    excess = int((flat[over] - cap).sum())
    assert seg == min(max((excess // 2048 + 63) // 64 * 64, p['seg_min']), p['seg_max']), (what, seg, excess)
    assert tasks.shape[0] == dyn['n_tasks'] and obs.shape[0] == dyn['n_obs']
    if over.size == 0:
        assert dyn['n_tasks'] == 0 and dyn['n_obs'] == 0, (what, dyn)
    else:
        assert np.isin(tasks[:, 0], over).all(), (what, 'a task of a bucket that is not oversized')
        size = flat[tasks[:, 0]]
        lo = cap + tasks[:, 1] * seg
        hi = np.minimum(lo + seg, size)
        assert (lo < hi).all(), (what, 'an empty segment')
        order = np.lexsort((lo, tasks[:, 0]))
        g, lo, hi = tasks[order, 0], lo[order], hi[order]
        first = np.r_[True, g[1:] != g[:-1]]
        last = np.r_[first[1:], True]
        assert np.array_equal(g[first], over), (what, 'oversized buckets without tasks')
        assert (lo[first] == cap).all() and (hi[last] == flat[g[last]]).all() and (lo[1:][~first[1:]] == hi[:-1][~first[1:]]).all(), (what, 'segments do not tile [cap, size)')
        # fold groups: their task ranges partition [0, n_tasks); one per bucket (merged: per bucket index, shared by the windows)
        ob = obs[np.argsort(obs[:, 1])]
        assert (ob[:, 2] > 0).all() and ob[0, 1] == 0 and (ob[1:, 1] == ob[:-1, 1] + ob[:-1, 2]).all() and ob[-1, 1] + ob[-1, 2] == dyn['n_tasks'], (what, 'fold groups')
        group_of_task = np.repeat(ob[:, 0], ob[:, 2])
        assert np.array_equal(group_of_task, tasks[:, 0] % B if merged else tasks[:, 0]), (what, 'a task outside its fold group')
        assert np.array_equal(np.sort(ob[:, 0]), np.unique(over % B) if merged else over), (what, 'one fold group per bucket')
    # ---- size order and the addition count
    clipped = np.minimum(totals, cap)
    if merged:
        mt = clipped.sum(axis=0)
        assert np.array_equal(d['mt'], mt), (what, 'merged lengths')
        check_size_order(d['perm'].astype(np.int64), mt, min(cap * W, 1 << 30), what)
        assert dyn['adds'] == int(np.maximum(mt - 1, 0).sum()), (what, 'adds')
    else:
        check_size_order(d['perm'].astype(np.int64), flat, cap, what)
        assert dyn['adds'] == int(np.maximum(clipped - 1, 0).sum()), (what, 'adds')
    return p, dyn


# ------------------------------------------------------------------------------------------ scalar classes (canonical integers)
def uniform(rng, n):
    return [int.from_bytes(rng.bytes(40), 'little') % R for _ in range(n)]


def witness(rng, n):
    """the project's 'witness' distribution (helpers.rand_fr_mont): a quarter zeros, a quarter ones, the rest uniform"""
    sel = rng.integers(0, 4, size=n)
    return [0 if s == 0 else 1 if s == 1 else v for s, v in zip(sel, uniform(rng, n))]


def nonzero_digits(rng, n, p):
    """every window's digit positive and non-zero (raw in [1, 2^(cw-1)], the top window's small enough for s < r): no entry drops out of
    the sort, so with one high bin a window's single segment holds all n entries"""
    win = windows(p)
    out = [0] * n
    for w, (o, cw) in enumerate(win):
        top = (1 << (cw - 1)) if w + 1 < len(win) else max(1, 1 << (cw - 3))
        for i, r in enumerate(rng.integers(1, top + 1, size=n)):
            out[i] |= int(r) << o
    assert max(out) < R
    return out


def digit_edges(p):
    """0, 1, r-1, 2^253 - 1 (every window all ones: the carry runs through all W windows); per window: raw digit exactly 2^(cw-1) (stays
    positive) and 2^(cw-1) + 1 (the first negative one); a single bit at each window's first and last position (windows that straddle a
    32-bit limb and the one that contains limb 7 among them)"""
    out = [0, 1, R - 1, (1 << 253) - 1]
    for o, cw in windows(p):
        out += [v for v in ((1 << (cw - 1)) << o, ((1 << (cw - 1)) + 1) << o, 1 << o, 1 << (o + cw - 1)) if v < R]
    return out


def skew_768(rng, p, cap_min):
    """bucket sizes 767, 768, 769 (and 1, 766, 770, and 2000: above the cap) side by side: a small scalar v <= 2^(cw-1) is window 0's
    positive digit v, i.e. bucket v - 1, and nothing anywhere else"""
    assert p['cap'] >= cap_min and 7 <= 1 << (windows(p)[0][1] - 1)
    out = []
    for v, copies in ((1, 767), (2, 768), (3, 769), (4, 1), (5, 766), (6, 770), (7, 2000)):
        out += [v] * copies
    rng.shuffle(out)
    return out


# ------------------------------------------------------------------------------------------ cases
def _case(kind, n, wb, merged, seed=1):
    from fawkes_crypto_amd import api
    rng = np.random.default_rng(seed * 1000003 + n * 31 + wb)
    p = api.msm_plan(n, wb, merged)
    if kind == 'uniform':
        v = uniform(rng, n)
    elif kind == 'witness':
        v = witness(rng, n)
    elif kind == 'nonzero':
        v = nonzero_digits(rng, n, p)
    elif kind == 'edges':
        v = digit_edges(p)
        assert len(v) <= n
        v = (v * (n // len(v) + 1))[:n]
    elif kind == 'equal':
        v = nonzero_digits(rng, 1, p) * n          # one bucket in EVERY window
    elif kind == 'halves':
        v = [1] * (n // 2) + [uniform(rng, 1)[0]] * (n - n // 2)
        rng.shuffle(v)
    elif kind == 'zero':
        v = [0] * n
    elif kind == 'repeat8':
        v = uniform(rng, n // 8) * 8
    elif kind == 'knee':
        v = skew_768(rng, p, 1000)
    assert len(v) == n, (kind, n, len(v))
    return mont(v)


CASES = (
    # ragged n: odd n leaves the second scalar of the digits kernel's last lane unused
    [('uniform', n, 0, False) for n in (1, 2, 3, 63, 64, 65)] + [('witness', 65, 12, False), ('witness', 3, 2, False)]
    # 8192 entries per first-pass sub-tile and per second-pass tile; c <= 11: one segment per window holds every entry
    + [('nonzero', n, 8, False) for n in (8191, 8192, 8193)] + [('uniform', 8193, 3, False), ('witness', 8193, 11, False)]
    # 16 384 entries per first-pass chunk: 1, 2, 3 and 4 chunks, the last one short or full
    + [('uniform', n, 12, False) for n in (16383, 16384, 16385, 32769, 49152)] + [('nonzero', 16385, 11, False), ('witness', 16385, 8, False)]
    # window bits: 2 (windows of 2 and 1 bits), 3, 8, 11, 12 (1 -> 2 high bins), 17, 21, 22 (2048 low bins)
    + [('witness', 1000, wb, False) for wb in (2, 3, 8, 11, 12, 17, 21, 22)] + [('uniform', 33000, 17, False)]
    # digit boundaries, carry chain, single bits at the window edges -- under narrow, limb-straddling and widest windows
    + [('edges', 600, wb, False) for wb in (2, 3, 8, 11, 12, 17, 21, 22)]
    # skew
    + [('equal', 700, 8, False), ('equal', 300000, 8, False), ('equal', 12001, 17, False), ('halves', 12000, 12, False), ('repeat8', 48000, 12, False),
       ('repeat8', 48000, 17, False), ('knee', 5841, 4, False), ('zero', 5000, 12, False), ('zero', 1, 0, False)]
    # merged form (one bucket set over all windows)
    + [('witness', 16385, 12, True), ('halves', 12000, 17, True), ('edges', 600, 22, True), ('repeat8', 48000, 0, True)]
)


@pytest.mark.parametrize('kind,n,wb,merged', CASES, ids=['%s-n%d-c%d%s' % (k, n, wb, '-merged' if m else '') for k, n, wb, m in CASES])
def test_front(ctx, kind, n, wb, merged):
    p, dyn = check_front(ctx, _case(kind, n, wb, merged), wb, merged, (kind, n, wb, merged))
    assert p['W'] * n <= 2200000 or (kind, n) == ('equal', 300000)          # the reference stays quick (SEG_MAX needs 8.3 M oversized entries)
    if kind == 'equal':                   # one bucket per window holds all n entries: W oversized buckets, seg clamped by n
        assert dyn['n_over'] == p['W'] and dyn['n_obs'] == p['W'] and dyn['cap'] == p['cap']
        assert dyn['seg'] == (p['seg_min'] if n == 700 else p['seg_max'] if n == 300000 else dyn['seg'])
    if kind == 'repeat8' and not merged and wb == 17:
        assert dyn['cap'] > p['cap']      # thousands of buckets of 8 over a statistical cap below 8: the cap doubles
    if kind == 'knee':
        assert dyn['cap'] > 769 and dyn['n_over'] >= 1
    if kind == 'zero':
        assert dyn['n_over'] == 0 and dyn['adds'] == 0


def test_the_cases_reach_the_boundaries_they_name():
    """host only (fk_msm_plan): the plans behind the cases above are the ones their comments claim"""
    from fawkes_crypto_amd import api
    assert api.msm_plan(1000, 2)['cb'] == 1 and api.msm_plan(1000, 2)['c'] == 2
    assert api.msm_plan(1000, 11)['nhi'] == 1 and api.msm_plan(1000, 12)['nhi'] == 2 and api.msm_plan(1000, 22)['nlo'] == 2048
    assert api.msm_plan(1000, 21)['nhi'] == 512 and api.msm_plan(1000, 17)['L'] >= 2 and api.msm_plan(1000, 22)['L'] == 64
    p = api.msm_plan(16385, 12)
    assert p['chunk'] == 16384 and p['nchunks'] == 2 and api.msm_plan(49152, 12)['nchunks'] == 3 and p['s1_tile'] == p['s2_tile'] == 8192
    assert 769 < api.msm_plan(5841, 4)['cap'] < 2000
    # windows that straddle a 32-bit limb, and one that contains bits of limb 7
    for wb in (3, 11, 17, 22):
        win = windows(api.msm_plan(300, wb))
        assert any(o // 32 != (o + cw - 1) // 32 for o, cw in win) and any(o + cw - 1 >= 224 for o, cw in win)


def test_dump_twice_with_a_multiplication_in_between(ctx, oracle):
    """the dump leaves the lanes usable, buffer growth does not corrupt it, and the multiplication after it does not adopt its sort"""
    rng = np.random.default_rng(77)
    a, b = mont(witness(rng, 3000)), mont(witness(rng, 20001))
    check_front(ctx, a, 12, False, 'first dump')
    bases = g1_bases(500, seed=3)
    sc = mont(witness(rng, 500))
    assert ctx.msm_g1(bases, sc).tobytes() == oracle.msm_g1(bases, sc).tobytes()
    check_front(ctx, b, 12, False, 'second, larger dump')
    check_front(ctx, a, 0, True, 'third dump, merged, on the next lane')
    assert ctx.msm_g1(bases, sc).tobytes() == oracle.msm_g1(bases, sc).tobytes()


def test_dump_of_nothing_and_of_too_much(ctx):
    """n == 0 and n >= 2^31 answer as a multiplication does: nothing to do, and FK_ERR_BAD_ARG"""
    import ctypes as C
    import fawkes_crypto_amd as fk
    d = ctx.msm_front_dump(np.zeros((0, 4), np.uint64))
    assert d['dyn']['n_tasks'] == 0 and d['digits'].shape[1] == 0
    one = np.zeros(4, np.uint32)
    dyn = fk.api.MsmDynInfo()
    d_s = ctx.dev_alloc(64)
    try:
        rc = ctx.lib.fk_msm_front_dump(ctx.handle, C.c_void_p(d_s), C.c_size_t(1 << 31), C.c_int(0), *[C.c_void_p(one.ctypes.data)] * 5, C.byref(dyn),
                                       C.c_void_p(one.ctypes.data), C.c_size_t(0), C.c_void_p(one.ctypes.data), C.c_size_t(0))
    finally:
        ctx.dev_free(d_s)
    assert rc == 1 and b'n too large' in ctx.lib.fk_last_error(ctx.handle)
