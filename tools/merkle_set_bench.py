#!/usr/bin/env python3
"""Bulk leaf writes (include/fawkes_hip_merkle_set.h) beside the ordered update with all outputs NULL -- the only other way to bring a
list of leaves into a tree on the device -- on the same inputs, in one run.  t = 3 parameters (3, 8, 53).

Sparse, depth 32, the tables sized up front: k in --writes, and two index sets: `uniform` (random below 2^32) and `contiguous`
(0 .. k - 1: accounts allocated one after the other, the restore and genesis case).  Per index set and k, for the set and for the update:
  first      the first call on an empty tree (fk_smt_set_timed_dev / fk_smt_update_timed_dev: the device time of the whole call): every
             node is inserted.  For the set this is the RESTORE of a tree of k leaves; for the update it is what populating cost before
  again      the same writes again -- the same sorts, probes and hashes, every node already stored: a host clock around a stream
             synchronise over windows of at least --window seconds, --repeats windows: min / median / max
  device     the timed entry's two figures for one such call (median of --repeats): the whole call and its hash launches alone, and the
             share of the call that is not a hash launch
  hashes     the set's: the sum of the distinct touched nodes of levels 1 .. depth as the timed entry returns them; the update's: k x depth;
             and hashes per second of the `again` median
Dense, depth 24, all 2^24 leaves populated, k in --dense-writes, uniform indices: the set, the update with all outputs NULL, and a rebuild
of the whole tree from its leaves (fk_poseidon_merkle_tree_dev).
The last line is one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import merkle, merkle_set  # noqa: E402
from fawkes_crypto_amd.sparse_merkle import SparseMerkleTree  # noqa: E402
from poseidon_bench import timed  # noqa: E402

T, F, P = 3, 8, 53


def median_of(call, repeats):
    """call() -> a tuple led by the two device times; the tuple with the median whole-call time"""
    got = sorted((call() for _ in range(repeats)), key=lambda r: r[0])
    return got[len(got) // 2]


def fmt3(seconds):
    return '%9.3f / %9.3f / %9.3f ms' % tuple(s * 1e3 for s in seconds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--depth', type=int, default=32)
    ap.add_argument('--dense-depth', type=int, default=24)
    ap.add_argument('--writes', default='1741,65536,1048576,16777216')
    ap.add_argument('--dense-writes', default='65536,1048576')
    args = ap.parse_args()
    depth, dd = args.depth, args.dense_depth
    writes = [int(x) for x in args.writes.split(',')]
    dense_writes = [int(x) for x in args.dense_writes.split(',')]
    kmax = max(writes + dense_writes)
    ctx = fk.Context(0)
    pp = fk.PoseidonParams(T, F, P)
    rng = np.random.default_rng(32)
    res = dict(depth=depth, dense_depth=dd, window_s=args.window, repeats=args.repeats, sparse={}, dense={})
    print('library %s   sparse depth %d   dense depth %d   windows of %.2f s x %d: min / median / max' % (os.path.basename(fk.lib_path()), depth, dd, args.window, args.repeats))
    d_idx, d_new = ctx.dev_alloc(8 * kmax), ctx.dev_alloc(32 * kmax)
    ctx.gen_scalars_dev(d_new, kmax, 13)

    for name in ('uniform', 'contiguous'):
        res['sparse'][name] = {}
        for k in writes:
            idx = rng.integers(0, 1 << depth, k, dtype=np.uint64) if name == 'uniform' else np.arange(k, dtype=np.uint64)
            ctx.upload(d_idx, idx)
            row = res['sparse'][name][k] = {}
            # the set: first call (restore), then the same writes again
            tree = SparseMerkleTree(ctx, pp, depth, k)
            first_ms, _, distinct = merkle_set.set_sparse_timed_dev(tree, d_idx, d_new, k)
            set_s, _ = timed(ctx, lambda: merkle_set.set_sparse_dev(tree, d_idx, d_new, k), args.window, args.repeats)
            set_ms, set_hash_ms, _ = median_of(lambda: merkle_set.set_sparse_timed_dev(tree, d_idx, d_new, k), args.repeats)
            root = tree.root_limbs()
            tree.free()
            set_hashes = sum(distinct[1:])
            row['set'] = dict(hashes=set_hashes, distinct=distinct, first_ms=first_ms, again_ms=[s * 1e3 for s in set_s], device_ms=set_ms, hash_launches_ms=set_hash_ms,
                              not_hashing_ms=set_ms - set_hash_ms, hashes_per_s=set_hashes / set_s[1])
            # the ordered update with all outputs NULL on the same inputs
            tree = SparseMerkleTree(ctx, pp, depth, k)
            ufirst_ms, _ = tree.update_timed_dev(d_idx, d_new, k, None, None, None)
            upd_s, _ = timed(ctx, lambda: tree.update_dev(d_idx, d_new, k, None, None, None), args.window, args.repeats)
            upd_ms, upd_hash_ms = median_of(lambda: tree.update_timed_dev(d_idx, d_new, k, None, None, None), args.repeats)
            same = tree.root_limbs().tobytes() == root.tobytes()
            tree.free()
            upd_hashes = k * depth
            row['update'] = dict(hashes=upd_hashes, first_ms=ufirst_ms, again_ms=[s * 1e3 for s in upd_s], device_ms=upd_ms, hash_launches_ms=upd_hash_ms,
                                 not_hashing_ms=upd_ms - upd_hash_ms, hashes_per_s=upd_hashes / upd_s[1])
            row['same_root'] = same
            row['hash_ratio'], row['time_ratio'], row['first_ratio'] = upd_hashes / set_hashes, upd_s[1] / set_s[1], ufirst_ms / first_ms
            print('sparse %-10s k %8d  set     %10d hashes  first %10.3f ms  again %s (%.4g hashes/s)  device %9.3f ms: hash launches %9.3f, the rest %8.3f'
                  % (name, k, set_hashes, first_ms, fmt3(set_s), set_hashes / set_s[1], set_ms, set_hash_ms, set_ms - set_hash_ms))
            print('sparse %-10s k %8d  update  %10d hashes  first %10.3f ms  again %s (%.4g hashes/s)  device %9.3f ms: hash launches %9.3f, the rest %8.3f'
                  % (name, k, upd_hashes, ufirst_ms, fmt3(upd_s), upd_hashes / upd_s[1], upd_ms, upd_hash_ms, upd_ms - upd_hash_ms))
            print('sparse %-10s k %8d  update / set: hashes %.2fx  again (median) %.2fx  first %.2fx  roots equal: %s' % (name, k, row['hash_ratio'], row['time_ratio'], row['first_ratio'], same))
        wins = [k for k in writes if res['sparse'][name][k]['time_ratio'] > 1]
        print('sparse %-10s the set is faster than the update (again, median) at k in %s of %s' % (name, wins, writes))

    n = 1 << dd
    d_nodes = ctx.dev_alloc(32 * (2 * n - 1))
    ctx.gen_scalars_dev(d_nodes, n, 11)
    ctx.merkle_tree_dev(pp, d_nodes, n, d_nodes)
    for k in dense_writes:
        ctx.upload(d_idx, rng.integers(0, n, k, dtype=np.uint64))
        _, _, distinct = merkle_set.set_dense_timed_dev(ctx, pp, d_nodes, dd, d_idx, d_new, k)
        set_s, _ = timed(ctx, lambda: merkle_set.set_dense_dev(ctx, pp, d_nodes, dd, d_idx, d_new, k), args.window, args.repeats)
        upd_s, _ = timed(ctx, lambda: merkle.update_dev(ctx, pp, d_nodes, dd, d_idx, d_new, k, None, None, None), args.window, args.repeats)
        reb_s, _ = timed(ctx, lambda: ctx.merkle_tree_dev(pp, d_nodes, n, d_nodes), args.window, args.repeats)
        set_hashes = sum(distinct[1:])
        res['dense'][k] = dict(set=dict(hashes=set_hashes, again_ms=[s * 1e3 for s in set_s]), update=dict(hashes=k * dd, again_ms=[s * 1e3 for s in upd_s]),
                               rebuild=dict(hashes=n - 1, again_ms=[s * 1e3 for s in reb_s]))
        print('dense  2^%d      k %8d  set %10d hashes %s   update %10d hashes %s   rebuild %10d hashes %s'
              % (dd, k, set_hashes, fmt3(set_s), k * dd, fmt3(upd_s), n - 1, fmt3(reb_s)))
    for d in (d_nodes, d_idx, d_new):
        ctx.dev_free(d)
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
