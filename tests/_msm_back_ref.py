"""Support of tests/test_gpu_msm_back.py: the ctypes side of fk_msm_back_dump (include/fawkes_hip_inspect.h: test-only, so its prototype is
declared here) and the reference every stage of the back of a multiplication is compared with.

Group elements are held as the raw affine bytes the oracle speaks (Montgomery x || y little endian, infinity all zero: what the device
holds as an Affine).  A device Xyzz is normalised in Python integers (x / zz, y / zzz mod p; zz = 0: infinity) and compared as bytes, so
every comparison is exact.  Sums come from the C oracle: a run of entries is ONE msm call with unit scalars (a negative entry's base is
negated here: -y mod p), a weighted sum one call with the small weights.  Every stage is compared twice: with the reference applied to
what the device left one stage earlier (a failure names the stage), and with the reference chain from the bases and the reference digits
of the scalars (tests/test_gpu_msm_front.py: ref_digits).  In the merged form the chain takes window w's points from the device's levels,
which check_levels ties to the bases first."""
import ctypes as C

import numpy as np

import bn254_ref as ref
import c_oracle as co
from helpers import Q, R
from test_gpu_msm_front import mont, ref_digits, windows

BUCKETS_CAP = 1 << 20            # bucket sets up to this many buckets are copied out (c <= 17 in the ordinary form)
MONT_Q = (1 << 256) % Q
Q_LIMBS = np.frombuffer(Q.to_bytes(32, 'little'), np.uint64)


class BackOut(C.Structure):
    """fk_msm_back_out"""
    _fields_ = [('sorted', C.c_void_p), ('starts', C.c_void_p), ('totals', C.c_void_p), ('perm', C.c_void_p), ('dyn', C.c_void_p),
                ('tasks', C.c_void_p), ('tasks_cap', C.c_size_t), ('obs', C.c_void_p), ('obs_cap', C.c_size_t),
                ('buckets_acc', C.c_void_p), ('buckets', C.c_void_p), ('buckets_cap', C.c_size_t), ('partials', C.c_void_p), ('partials_cap', C.c_size_t),
                ('winparts', C.c_void_p), ('folded', C.c_void_p), ('result', C.c_void_p), ('levels', C.c_void_p)]


def entry(lib):
    fn = lib.fk_msm_back_dump
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(BackOut)]
    return fn


def small_mont(ks):
    return co.limbs_arr([(int(k) << 256) % R for k in ks])


def below_q(limbs):
    """limbs (..., 4) uint64 little endian -> value < q, elementwise"""
    lt, eq = np.zeros(limbs.shape[:-1], bool), np.ones(limbs.shape[:-1], bool)
    for j in (3, 2, 1, 0):
        lt |= eq & (limbs[..., j] < Q_LIMBS[j])
        eq &= limbs[..., j] == Q_LIMBS[j]
    return lt


class Group:
    """G1 or G2 over raw affine bytes"""

    def __init__(self, g2):
        self.g2, self.pb, self.k = bool(g2), 128 if g2 else 64, 2 if g2 else 1          # bytes of an affine point, base-field values per coordinate
        self.curve, self.F = (ref.G2, ref.F2) if g2 else (ref.G1, ref.F1)
        self._msm, self._add, self._mul = (co.msm_g2, co.g2_add, co.g2_mul) if g2 else (co.msm_g1, co.g1_add, co.g1_mul)
        self.inf = bytes(self.pb)
        self._ones = small_mont([1] * 4096)

    def sum(self, pts):
        m = len(pts)
        if m == 0:
            return self.inf
        if m > len(self._ones):
            self._ones = small_mont([1] * (2 * m))
        return self._msm(pts, self._ones[:m]).tobytes()

    def msm(self, pts, ks):
        return self._msm(pts, small_mont(ks)).tobytes() if len(pts) else self.inf

    def add(self, p, q):
        if p == self.inf:
            return q
        if q == self.inf:
            return p
        return self._add(np.frombuffer(p, np.uint8), np.frombuffer(q, np.uint8)).tobytes()

    def mul_pow2(self, p, k):
        return p if p == self.inf else self._mul(np.frombuffer(p, np.uint8), small_mont([1 << k])[0]).tobytes()

    def negate(self, pts):
        """(m, pb) raw affine points -> their negatives (-y mod q in the Montgomery image; infinity stays)"""
        out = pts.copy()
        h = self.pb // 2
        for row in out:
            for o in range(h, self.pb, 32):
                v = int.from_bytes(row[o:o + 32].tobytes(), 'little')
                if v:
                    row[o:o + 32] = np.frombuffer((Q - v).to_bytes(32, 'little'), np.uint8)
        return out

    def nonzero(self, xyzz):
        """(m, 2 pb) device Xyzz -> zz != 0"""
        return xyzz[:, self.pb:self.pb + self.pb // 2].any(axis=1)

    def canonical(self, xyzz):
        """every coordinate of every point is a residue below q"""
        return bool(below_q(np.ascontiguousarray(xyzz).view(np.uint64).reshape(-1, 4)).all())

    def norm(self, xyzz):
        """(m, 2 pb) device Xyzz (Montgomery limb images) -> (m, pb) raw affine: leaves Montgomery form, x / zz, y / zzz, back to raw"""
        out = np.zeros((len(xyzz), self.pb), np.uint8)
        F, k = self.F, self.k
        for i in np.nonzero(self.nonzero(xyzz))[0]:
            v = [int.from_bytes(xyzz[i, o:o + 32].tobytes(), 'little') for o in range(0, 2 * self.pb, 32)]
            x, y, zz, zzz = (tuple(v[j * k:(j + 1) * k]) if k == 2 else v[j] for j in range(4))
            # a quotient of two Montgomery images is the canonical quotient; times 2^256: its Montgomery image
            ax, ay = F.muli(F.mul(x, F.inv(zz)), MONT_Q), F.muli(F.mul(y, F.inv(zzz)), MONT_Q)
            vals = (ax + ay) if k == 2 else (ax, ay)
            out[i] = np.frombuffer(b''.join(int(c).to_bytes(32, 'little') for c in vals), np.uint8)
        return out

    def from_raw(self, b):
        return (ref.g2_from_raw_le if self.g2 else ref.g1_from_raw_le)(bytes(b))


def run_dump(ctx, g2, bases, ints, wb, merged):
    """one fk_msm_back_dump of host bases ((n, pb) raw affine) and canonical integer scalars under `wb` forced window bits -> dict"""
    from fawkes_crypto_amd import api
    G = Group(g2)
    n = len(ints)
    assert bases.shape == (n, G.pb)
    p = api.msm_plan(n, wb, merged)
    W, B = p['W'], p['B']
    WR = 1 if merged else W
    nb = WR * B
    xb = 2 * G.pb
    tasks_cap = W * n // p['seg_min'] + p['over_max'] + 1
    d = dict(G=G, plan=p, n=n, merged=merged, WR=WR, bases=bases, ints=list(ints), scalars=mont(ints) if n else np.zeros((0, 4), np.uint64),
             sorted=np.zeros((W, n), np.uint32), starts=np.zeros((W, B), np.uint32), totals=np.zeros((W, B), np.uint32),
             perm=np.zeros(2 * B if merged else W * B, np.uint32), tasks=np.zeros((tasks_cap, 2), np.uint32), obs=np.zeros((p['over_max'], 3), np.uint32),
             partials=np.zeros((tasks_cap, xb), np.uint8), winparts=np.zeros((WR * p['nblk'], xb), np.uint8), folded=np.zeros((WR, xb), np.uint8),
             result=np.zeros((1, xb), np.uint8), levels=np.zeros((W - 1, n, G.pb), np.uint8) if merged else None,
             buckets_acc=np.zeros((nb, xb), np.uint8) if nb <= BUCKETS_CAP else None, buckets=np.zeros((nb, xb), np.uint8) if nb <= BUCKETS_CAP else None)
    dyn = api.MsmDynInfo()
    out = BackOut()
    for f in ('sorted', 'starts', 'totals', 'perm', 'tasks', 'obs', 'partials', 'winparts', 'folded', 'result', 'levels', 'buckets_acc', 'buckets'):
        setattr(out, f, d[f].ctypes.data if d[f] is not None else None)
    out.dyn = C.addressof(dyn)
    out.tasks_cap = out.partials_cap = tasks_cap
    out.obs_cap, out.buckets_cap = p['over_max'], BUCKETS_CAP
    d_b, d_s = ctx.dev_alloc(max(n, 1) * G.pb), ctx.dev_alloc(max(n, 1) * 32)
    ctx.set_window_bits(wb)
    try:
        if n:
            ctx.upload(d_b, bases)
            ctx.upload(d_s, d['scalars'])
        ctx.msm_back_dump(entry(ctx.lib), out, d_b, d_s, n, g2=g2, merged=merged)
    finally:
        ctx.set_window_bits(0)
        ctx.dev_free(d_b)
        ctx.dev_free(d_s)
    d['dyn'] = {f: int(getattr(dyn, f)) for f, _ in api.MsmDynInfo._fields_}
    assert d['dyn']['n_tasks'] <= tasks_cap and d['dyn']['n_obs'] <= p['over_max'], d['dyn']
    d['tasks'], d['obs'], d['partials'] = d['tasks'][:d['dyn']['n_tasks']], d['obs'][:d['dyn']['n_obs']], d['partials'][:d['dyn']['n_tasks']]
    return d


class Back:
    """The stages of one dump against their references.  check() runs them all in the order of the pipeline; every assertion message
    opens with the stage it belongs to."""

    def __init__(self, d, what):
        self.d, self.what, self.G = d, what, d['G']
        self.p, self.dyn, self.merged, self.n = d['plan'], d['dyn'], d['merged'], d['n']
        self.W, self.B, self.WR = self.p['W'], self.p['B'], d['WR']
        self.win = windows(self.p)
        _, self.mag, self.neg = ref_digits(d['scalars'], self.p)
        # reference runs: window w's entries ordered by digit; the entries of bucket b are order[bounds[b] : bounds[b + 1]]
        self.order = [np.argsort(self.mag[w], kind='stable') for w in range(self.W)]
        digits = np.arange(1, self.B + 2)
        self.bounds = [np.searchsorted(self.mag[w][self.order[w]], digits).astype(np.int32) for w in range(self.W)]
        self.have_buckets = d['buckets'] is not None

    # ---- points
    def level(self, w):
        return self.d['levels'][w - 1] if (self.merged and w) else self.d['bases']

    def points(self, w, idx, neg):
        pts = self.level(w)[idx]
        if neg.any():
            pts[neg] = self.G.negate(pts[neg])
        return pts

    def dev_run(self, w, b, lo, hi):
        """entries [lo, hi) of the device's sorted run of bucket (w, b) as points (bit 31 of an entry negates its base)"""
        s = int(self.d['starts'][w, b])
        e = self.d['sorted'][w, s + lo:s + hi]
        return self.points(w, (e & 0x7fffffff).astype(np.int64), (e >> 31).astype(bool))

    def ref_run(self, w, lo, hi):
        """the reference digits' entries of buckets [lo, hi) of window w: (points, digit magnitudes)"""
        idx = self.order[w][self.bounds[w][lo]:self.bounds[w][hi]]
        return self.points(w, idx, self.neg[w][idx]), self.mag[w][idx]

    def sets(self, r):
        """the windows that feed bucket set r"""
        return range(self.W) if self.merged else (r,)

    def fail(self, stage, bad, total):
        assert not bad, '%s: %s: %d of %d wrong, first: %s' % (stage, self.what, len(bad), total, bad[:4])

    # ---- stages
    def check_levels(self):
        """levels[w-1][i] = 2^(offset_w) * bases[i], canonical affine, infinity stays infinity.  Every level is compared with 2^bits times
        the level below it (G1: every point, doubled in Python integers and compared projectively; G2, whose doublings cost five times as
        much, beyond 64 points: the first and last groups, the points around each block boundary, infinities and their neighbours,
        every 16th point) and the top level with the oracle's 2^offset * base for EVERY point: doubling is injective on a group of odd
        order, so a wrong point at any level shows at the top one as well.  Beyond 2048 points (the overflow cases, which are not about
        the level kernel) both comparisons take the same selection with a stride of n / 256; the multiplication's result, compared
        with the oracle's, depends on every level point whose digit is not zero."""
        if not self.merged:
            return
        G, n, lev, bases = self.G, self.n, self.d['levels'], self.d['bases']
        curve, F = G.curve, G.F
        assert bool(below_q(np.ascontiguousarray(lev).view(np.uint64).reshape(-1, 4)).all()), 'levels: %s: a coordinate is not below q' % (self.what,)
        inf0 = ~bases.any(axis=1)
        pick = np.ones(n, bool)
        if (G.g2 and n > 64) or n > 2048:
            pick[:] = False
            near = [0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1] + [k * 512 + j for k in range(1, n // 512 + 1) for j in (-2, -1, 0, 1)] + list(range(0, n, max(16, n // 256)))
            for i in np.nonzero(inf0)[0]:
                near += [i - 1, i, i + 1]
            pick[[i for i in near if 0 <= i < n]] = True
        bad = []
        for w in range(1, self.W):
            below, cur, bits = self.level(w - 1), lev[w - 1], self.win[w - 1][1]
            inf = ~cur.any(axis=1)
            if not np.array_equal(inf, inf0):
                bad.append(('level', w, 'infinity at', np.nonzero(inf != inf0)[0][:4].tolist()))
                continue
            for i in np.nonzero(pick & ~inf0)[0]:
                J = curve.to_jac(G.from_raw(below[i]))
                for _ in range(bits):
                    J = curve.jac_double(J)
                x, y = G.from_raw(cur[i])
                X, Y, Z = J
                z2 = F.sqr(Z)
                if F.mul(x, z2) != X or F.mul(y, F.mul(z2, Z)) != Y:
                    bad.append(('level', w, 'point', int(i)))
        top, off = lev[self.W - 2], self.win[self.W - 1][0]
        for i in (range(n) if n <= 2048 else np.nonzero(pick)[0]):
            if top[i].tobytes() != G.mul_pow2(bases[i].tobytes(), off):
                bad.append(('top level against the oracle, point', i))
        self.fail('levels', bad, (self.W - 1) * n)

    def bucket_runs(self, g):
        """bucket g of the bucket sets -> [(w, b)] runs that feed it"""
        if self.merged:
            return [(w, g) for w in range(self.W) if self.d['totals'][w, g]]
        return [divmod(g, self.B)]

    def check_accumulate(self):
        """buckets_acc[g] = the signed sum of the first min(totals, cap) entries of the device's run(s); an empty bucket is infinity; every
        coordinate stored is canonical"""
        if not self.have_buckets:
            return
        G, cap, acc = self.G, self.dyn['cap'], self.d['buckets_acc']
        assert G.canonical(acc), 'accumulate: %s: a stored coordinate is not below q (Walker::result)' % (self.what,)
        tot = self.d['totals'].astype(np.int64)
        length = tot.sum(axis=0) if self.merged else tot.reshape(-1)
        assert not acc[length == 0].any(), 'accumulate: %s: an empty bucket is not the all-zero infinity' % (self.what,)
        self.acc_norm = G.norm(acc)
        bad = []
        for g in np.nonzero(length)[0]:
            pts = np.concatenate([self.dev_run(w, b, 0, min(int(tot[w, b]), cap)) for w, b in self.bucket_runs(int(g))])
            if self.acc_norm[g].tobytes() != G.sum(pts):
                bad.append(('bucket', int(g), 'runs', [(w, b, int(tot[w, b])) for w, b in self.bucket_runs(int(g))], 'cap', cap))
        self.fail('accumulate', bad, int((length > 0).sum()))

    def check_partials(self):
        """partials[t] = the sum of entries [cap + seg * SEG, min(.. + SEG, size)) of task t's run, window w's bases from level w"""
        G, cap, SEG = self.G, self.dyn['cap'], self.dyn['seg']
        assert G.canonical(self.d['partials']), 'overflow partials: %s: a stored coordinate is not below q' % (self.what,)
        self.part_norm = G.norm(self.d['partials'])
        bad = []
        for t, (g, seg) in enumerate(self.d['tasks'].astype(np.int64)):
            w, b = divmod(int(g), self.B)
            lo = cap + int(seg) * SEG
            hi = min(lo + SEG, int(self.d['totals'][w, b]))
            if self.part_norm[t].tobytes() != G.sum(self.dev_run(w, b, lo, hi)):
                bad.append(('task', t, 'window', w, 'bucket', b, 'entries', lo, hi))
        self.fail('overflow partials', bad, len(self.d['tasks']))

    def check_fold(self):
        """buckets[g] = buckets_acc[g] + the sum of g's fold group; every other bucket is left as the accumulation stored it"""
        if not self.have_buckets:
            return
        G, buck, obs = self.G, self.d['buckets'], self.d['obs'].astype(np.int64)
        assert G.canonical(buck), 'overflow fold: %s: a stored coordinate is not below q' % (self.what,)
        untouched = np.ones(len(buck), bool)
        untouched[obs[:, 0]] = False
        assert np.array_equal(buck[untouched], self.d['buckets_acc'][untouched]), 'overflow fold: %s: a bucket outside every fold group changed' % (self.what,)
        self.buck_norm = self.acc_norm.copy()
        self.buck_norm[obs[:, 0]] = G.norm(buck[obs[:, 0]])
        bad = []
        for g, t0, nt in obs:
            want = G.add(self.acc_norm[g].tobytes(), G.sum(self.part_norm[t0:t0 + nt]))
            if self.buck_norm[g].tobytes() != want:
                bad.append(('bucket', int(g), 'tasks', int(t0), int(nt)))
        self.fail('overflow fold', bad, len(obs))

    def check_buckets_chain(self):
        """the buckets behind the fold against the reference digits: bucket (w, b) holds every base whose digit in window w is +-(b + 1)"""
        if not self.have_buckets:
            return
        G, bad, cnt = self.G, [], 0
        for r in range(self.WR):
            sizes = sum(np.diff(self.bounds[w]) for w in self.sets(r))
            assert not self.d['buckets'][r * self.B:(r + 1) * self.B][sizes == 0].any(), 'buckets (chain): %s: a bucket no digit points to is not infinity' % (self.what,)
            for b in np.nonzero(sizes)[0]:
                pts = np.concatenate([self.ref_run(w, int(b), int(b) + 1)[0] for w in self.sets(r)])
                cnt += 1
                if self.buck_norm[r * self.B + b].tobytes() != G.sum(pts):
                    bad.append(('set', r, 'bucket', int(b), 'entries', len(pts)))
        self.fail('buckets (chain from the bases)', bad, cnt)

    def check_reduce(self):
        """winparts[r][blk] = the sum over the block's buckets of (s + 1) * bucket[r][s]: over the device's buckets, and over the reference
        digits' entries (digit * base)"""
        G, L, nblk, B = self.G, self.p['L'], self.p['nblk'], self.B
        assert self.p['T'] * L == B and nblk == (self.p['T'] + 255) // 256
        assert G.canonical(self.d['winparts']), 'reduce: %s: a stored coordinate is not below q' % (self.what,)
        self.wp_norm = G.norm(self.d['winparts'])
        bad, bad_chain = [], []
        for r in range(self.WR):
            for blk in range(nblk):
                lo, hi = blk * 256 * L, min((blk + 1) * 256 * L, B)
                got = self.wp_norm[r * nblk + blk].tobytes()
                if self.have_buckets:
                    s = np.nonzero(self.buck_norm[r * B + lo:r * B + hi].any(axis=1))[0]
                    if got != G.msm(self.buck_norm[r * B + lo + s], s + lo + 1):
                        bad.append(('set', r, 'block', blk, 'buckets', lo, hi, 'occupied', (s + lo)[:6].tolist()))
                runs = [self.ref_run(w, lo, hi) for w in self.sets(r)]
                if got != G.msm(np.concatenate([x[0] for x in runs]), np.concatenate([x[1] for x in runs])):
                    bad_chain.append(('set', r, 'block', blk, 'buckets', lo, hi))
        self.fail('reduce (winparts from the device buckets)', bad, self.WR * nblk)
        self.fail('reduce (winparts, chain from the bases)', bad_chain, self.WR * nblk)

    def check_folded(self):
        """folded[r] = the sum over the blocks of winparts[r]; chain: the sum over the entries of digit * base"""
        G, nblk = self.G, self.p['nblk']
        assert G.canonical(self.d['folded']), 'fold partials: %s: a stored coordinate is not below q' % (self.what,)
        self.fold_norm = G.norm(self.d['folded'])
        bad, bad_chain = [], []
        for r in range(self.WR):
            got = self.fold_norm[r].tobytes()
            if got != G.sum(self.wp_norm[r * nblk:(r + 1) * nblk]):
                bad.append(('set', r))
            runs = [self.ref_run(w, 0, self.B) for w in self.sets(r)]
            if got != G.msm(np.concatenate([x[0] for x in runs]), np.concatenate([x[1] for x in runs])):
                bad_chain.append(('set', r))
        self.fail('fold partials (folded from winparts)', bad, self.WR)
        self.fail('fold partials (folded, chain from the bases)', bad_chain, self.WR)

    def check_result(self):
        """Horner over folded with the plan's window widths (merged: the one sum is the result) = result = the oracle's multiplication"""
        G = self.G
        acc = G.inf
        for r in reversed(range(self.WR)):
            acc = G.add(G.mul_pow2(acc, self.win[r][1]), self.fold_norm[r].tobytes())
        got = G.norm(self.d['result'])[0].tobytes()
        assert got == acc, 'horner (msm_end over folded): %s' % (self.what,)
        assert got == G._msm(self.d['bases'], self.d['scalars']).tobytes(), 'result against the oracle: %s' % (self.what,)

    def check(self):
        assert self.dyn['error'] == 0, ('front', self.what, self.dyn)
        self.check_levels()
        self.check_accumulate()
        self.check_partials()
        self.check_fold()
        self.check_buckets_chain()
        self.check_reduce()
        self.check_folded()
        self.check_result()
        return self
