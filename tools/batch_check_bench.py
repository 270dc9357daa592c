#!/usr/bin/env python3
"""What the per-proof R1CS check costs inside the batch prover, in one run on one box.

  parent    batch.prove_batch_dev's C entry (fk_prove_batch_dev) from ANOTHER build of the library: --parent-lib, the commit before the check
  tree      fk_prove_batch_dev from this tree's library
  checked   fk_prove_batch_checked_dev from this tree's library: the same proofs plus one report per proof, the device bitmap and flags
            allocated once outside the timed calls (as a service would hold them)
  wrapper   batch.prove_batch_checked_dev, the Python wrapper of the same entry: it allocates and frees the two device arrays per call,
            downloads the bitmap when a gate is bad and builds `count` CheckReport objects -- host work, shown so that it is not taken
            for the check's cost

on BASELINE configs[0] (the depth-32 Poseidon Merkle proof: 7362 gates, domain 2^13) for count in --counts, the witnesses resident on the
device as rows.  Both libraries live in this one process, each with its own context, key and resident system (same toxic waste: the same
key).  Four distinct satisfying witnesses are dealt round robin; every --bad-every-th proof has one aux element redrawn, so the check has
something to find.  Before anything is timed, every method's proofs are compared byte by byte.

Timing: a host clock around the whole call (every method ends synchronised), one warm-up of every method at every count, then --rounds
rounds that ALTERNATE the methods; min / median / max milliseconds are printed.  `tree` is untouched code: it must lie within the parent's
own max - min of the parent's median.  The checked call's extra time is taken round by round (checked - tree of the same round; wrapper -
tree likewise) and printed beside check_ms (the check's device time, events around its four launches) and eval_ms of the same call -- the
stage that produces the bytes the check reads; an extra time above eval_ms is marked.  The last line is one JSON object.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import _abi, batch as B, check as K  # noqa: E402
import bn254_ref as ref  # noqa: E402
import fixtures as fx  # noqa: E402
from helpers import TOXIC  # noqa: E402
from batch_prove_bench import DISTINCT, config0  # noqa: E402

R = ref.R


class World:
    """one build of the library with its own context, key, resident system and witnesses"""

    def __init__(self, lib, r1cs, tox):
        self.lib = lib
        mine, fk.api._LIB = fk.api._LIB, lib            # Context() takes the library load_library() returns
        try:
            self.ctx = fk.Context(0)
        finally:
            fk.api._LIB = mine
        self.dk, _ = self.ctx.setup(r1cs, **tox)
        self.dr = self.ctx.load_r1cs(r1cs)
        self.d_z = None

    def witnesses(self, zs):
        if self.d_z:
            self.ctx.dev_free(self.d_z)
        self.d_z = self.ctx.dev_alloc(zs.nbytes)
        self.ctx.upload(self.d_z, zs)

    def prove(self, count, rs, ss, opts):
        """fk_prove_batch_dev -> (proofs, timings)"""
        out, tm = np.zeros((count, 256), np.uint8), B.BatchTimings()
        self.ctx._ck(self.lib.fk_prove_batch_dev(self.ctx.handle, self.dk.handle, self.dr.handle, self.d_z, B.Z_ROWS, count, rs.ctypes.data, ss.ctypes.data,
                                                 out.ctypes.data, C.byref(opts), C.byref(tm)))
        return out, tm.as_dict()

    def prove_checked(self, count, rs, ss, opts, d_bitmap, d_bad, sts):
        """fk_prove_batch_checked_dev into the caller's arrays -> (proofs, timings with check_ms)"""
        out, tm, ms = np.zeros((count, 256), np.uint8), B.BatchTimings(), C.c_double(0)
        self.ctx._ck(self.lib.fk_prove_batch_checked_dev(self.ctx.handle, self.dk.handle, self.dr.handle, self.d_z, B.Z_ROWS, count, rs.ctypes.data, ss.ctypes.data,
                                                         out.ctypes.data, C.byref(opts), C.byref(tm), d_bitmap, d_bad, sts, C.byref(ms)))
        return out, dict(tm.as_dict(), check_ms=ms.value)

    def close(self):
        if self.d_z:
            self.ctx.dev_free(self.d_z)
        self.dr.free(); self.dk.free(); self.ctx.close()


def load_parent(path):
    lib = C.CDLL(path)
    _abi.apply(lib)
    fn = lib.fk_prove_batch_dev
    fn.restype, fn.argtypes = B.PROTOTYPES['fk_prove_batch_dev'][0], list(B.PROTOTYPES['fk_prove_batch_dev'][1])
    return lib


def ms3(seconds):
    s = sorted(seconds)
    return [1e3 * s[0], 1e3 * s[len(s) // 2], 1e3 * s[-1]]


def three(values):
    s = sorted(values)
    return [s[0], s[len(s) // 2], s[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default='', help='libfawkes_hip.so built from the commit before the check; without it the parent is left out')
    ap.add_argument('--counts', default='64,1024')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--bad-every', type=int, default=8, help='every n-th proof gets a violated witness (0: none)')
    ap.add_argument('--budget-gib', type=float, default=64.0)
    args = ap.parse_args()
    counts = [int(x) for x in args.counts.split(',')]
    opts = B.BatchOpts(scratch_budget_bytes=int(args.budget_gib * 2 ** 30))
    tox = {k: fx.mont_fr(v) for k, v in TOXIC.items()}
    r1cs, distinct = config0()
    tree = World(B._lib(), r1cs, tox)
    parent = World(load_parent(args.parent_lib), r1cs, tox) if args.parent_lib else None
    methods = (['parent'] if parent else []) + ['tree', 'checked', 'wrapper']
    words = (r1cs.num_gates + 63) // 64
    c = tree.dk.counts()
    nv = c['num_input'] + c['num_aux']
    print('config0: domain 2^%d, %d gates, %d variables   methods %s   rounds %d (methods alternate)   ms: min / median / max'
          % (c['m'].bit_length() - 1, r1cs.num_gates, nv, ','.join(methods), args.rounds))
    if parent:
        print('parent library: %s' % args.parent_lib)
    res = dict(counts=counts, rounds=args.rounds, bad_every=args.bad_every, launches_added_per_group=B.CHECK_LAUNCHES, rows={})

    for count in counts:
        rnd = random.Random(count)
        zs = np.ascontiguousarray(np.stack([distinct[i % DISTINCT] for i in range(count)]))
        bad = [i for i in range(count) if args.bad_every and i % args.bad_every == args.bad_every - 1]
        for i in bad:
            zs[i, c['num_input'] + rnd.randrange(c['num_aux'])] = fx.mont_fr(rnd.randrange(2, R))
        rs = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in range(count)])
        ss = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in range(count)])
        for w in (tree, parent):
            if w:
                w.witnesses(zs)

        d_bitmap, d_bad = tree.ctx.dev_alloc(8 * words * count), tree.ctx.dev_alloc(max(count, 8))
        sts = (K.CheckReportStruct * count)()

        def wrapper():
            return B.prove_batch_checked_dev(tree.ctx, tree.dk, tree.dr, tree.d_z, B.Z_ROWS, count, rs, ss, opts=opts, want_timings=True)

        fns = dict(parent=(lambda: parent.prove(count, rs, ss, opts)), tree=(lambda: tree.prove(count, rs, ss, opts)),
                   checked=(lambda: tree.prove_checked(count, rs, ss, opts, d_bitmap, d_bad, sts)), wrapper=wrapper)
        # warm-up of every method at this count, and the comparison
        warm = {meth: fns[meth]() for meth in methods}
        for meth in methods:
            assert warm[meth][0].tobytes() == warm['tree'][0].tobytes(), '%s differs from this tree\'s unchecked proofs' % meth
        flagged = [i for i, rep in enumerate(warm['wrapper'][1]) if not rep.ok]
        assert set(flagged) <= set(bad), 'a satisfying witness was flagged'
        assert [i for i, st in enumerate(sts) if st.n_bad] == flagged and np.flatnonzero(tree.ctx.download(d_bad, count)).tolist() == flagged
        secs = {meth: [] for meth in methods}
        check_ms, eval_ms = [], []
        for _ in range(args.rounds):
            for meth in methods:
                t0 = time.perf_counter()
                out = fns[meth]()
                secs[meth].append(time.perf_counter() - t0)
                if meth == 'checked':
                    check_ms.append(out[1]['check_ms'])
                    eval_ms.append(out[1]['eval_ms'])
        tree.ctx.dev_free(d_bitmap); tree.ctx.dev_free(d_bad)
        row = res['rows'][count] = {meth: ms3(secs[meth]) for meth in methods}
        row['flagged'] = len(flagged)
        row['plan'] = B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], count, dict(scratch_budget_bytes=opts.scratch_budget_bytes))
        row['extra_ms'] = three([1e3 * (a - b) for a, b in zip(secs['checked'], secs['tree'])])
        row['wrapper_extra_ms'] = three([1e3 * (a - b) for a, b in zip(secs['wrapper'], secs['tree'])])
        row['check_ms'], row['eval_ms'] = three(check_ms), three(eval_ms)
        row['extra_above_eval'] = row['extra_ms'][1] > row['eval_ms'][1]
        print('count %5d   ' % count + '   '.join('%s %9.3f / %9.3f / %9.3f' % (meth, *row[meth]) for meth in methods)
              + '   groups %d x %d   flagged %d of %d violated' % (row['plan']['n_groups'], row['plan']['group'], len(flagged), len(bad)))
        if parent:
            spread = row['parent'][2] - row['parent'][0]
            row['tree_minus_parent_ms'] = row['tree'][1] - row['parent'][1]
            row['tree_within_parent_spread'] = abs(row['tree_minus_parent_ms']) <= spread
            print('              tree - parent (medians) %+.3f ms; the parent\'s own max - min %.3f ms: %s'
                  % (row['tree_minus_parent_ms'], spread, 'within' if row['tree_within_parent_spread'] else 'OUTSIDE'))
        print('              checked - tree, round by round %+.3f / %+.3f / %+.3f ms   check_ms %.3f / %.3f / %.3f   eval_ms %.3f / %.3f / %.3f%s'
              % (*row['extra_ms'], *row['check_ms'], *row['eval_ms'], '   EXTRA ABOVE eval_ms' if row['extra_above_eval'] else ''))
        print('              wrapper - tree, round by round %+.3f / %+.3f / %+.3f ms' % tuple(row['wrapper_extra_ms']))
    for w in (tree, parent):
        if w:
            w.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
