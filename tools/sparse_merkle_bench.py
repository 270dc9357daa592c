#!/usr/bin/env python3
"""Ordered leaf writes to a sparse Merkle tree in device memory (csrc/sparse_merkle.hip), t = 3 parameters (3, 8, 53): depth 32, 2^20 and
2^24 populated leaves (uniform random indices), and k uniform random writes, k in {1024, 2^16, 2^20}.  Per tree and k:
  update     fk_smt_update_dev with all three outputs (old leaves, siblings, roots): a host clock around a stream synchronise, after a
             warm-up, over a window of at least --window seconds, repeated --repeats times (median printed, min and max in the JSON).
             The warm-up is the call that inserts the writes' nodes (and grows the tables if it has to); the windows time the same writes
             again: the same probes and hashes, every node already stored
  hashes     its `depth` hash launches alone (fk_smt_update_timed_dev: HIP events around each launch; the sibling probe is inside), the
             median of --repeats timed calls, and what is left of the update's device time -- the index check, the sort, the plans, the
             write-backs, the copies -- as a share of it
  bytes      device bytes of the tree per stored node, after the writes
Beside them the yardstick: fk_poseidon_merkle_update_dev on a DENSE tree of depth 24 (2^24 leaves, all populated) with the same k.
The last line is one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import merkle  # noqa: E402
from fawkes_crypto_amd.sparse_merkle import SparseMerkleTree  # noqa: E402
from poseidon_bench import timed  # noqa: E402

T, F, P = 3, 8, 53


def median_timed(call, repeats):
    ev = sorted(call() for _ in range(repeats))
    return ev[len(ev) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--depth', type=int, default=32)
    ap.add_argument('--dense-depth', type=int, default=24)
    ap.add_argument('--populated', default='20,24', help='log2 of the populated leaves, one tree each')
    ap.add_argument('--writes', default='1024,65536,1048576')
    args = ap.parse_args()
    depth, dd = args.depth, args.dense_depth
    writes = [int(x) for x in args.writes.split(',')]
    kmax = max(writes)
    ctx = fk.Context(0)
    pp = fk.PoseidonParams(T, F, P)
    rng = np.random.default_rng(32)
    res = dict(depth=depth, dense_depth=dd, window_s=args.window, repeats=args.repeats, sparse={}, dense={})
    print('library %s   sparse depth %d   dense depth %d' % (os.path.basename(fk.lib_path()), depth, dd))
    d_idx, d_new, d_old, d_roots = (ctx.dev_alloc(b * kmax) for b in (8, 32, 32, 32))
    d_sib = ctx.dev_alloc(32 * kmax * max(depth, dd))
    ctx.gen_scalars_dev(d_new, kmax, 13)

    for lg in [int(x) for x in args.populated.split(',')]:
        n = 1 << lg
        tree = SparseMerkleTree(ctx, pp, depth, n + sum(writes))
        d_pi, d_pl = ctx.dev_alloc(8 * n), ctx.dev_alloc(32 * n)
        ctx.upload(d_pi, rng.integers(0, 1 << depth, n, dtype=np.uint64))
        ctx.gen_scalars_dev(d_pl, n, 11)
        pop_ms, _ = tree.update_timed_dev(d_pi, d_pl, n, None, None, None)
        ctx.dev_free(d_pi); ctx.dev_free(d_pl)
        info = tree.info()
        print('populated 2^%d leaves in %.1f ms: %d leaves, %d nodes stored, %.1f MB' % (lg, pop_ms, info['leaves'], info['nodes'], info['device_bytes'] / 1e6))
        rows = res['sparse'][lg] = dict(populate_ms=pop_ms, rows={})
        for k in writes:
            ctx.upload(d_idx, rng.integers(0, 1 << depth, k, dtype=np.uint64))
            upd, _ = timed(ctx, lambda: tree.update_dev(d_idx, d_new, k, d_old, d_sib, d_roots), args.window, args.repeats)
            dev_ms, hash_ms = median_timed(lambda: tree.update_timed_dev(d_idx, d_new, k, d_old, d_sib, d_roots), args.repeats)
            info = tree.info()
            other, per_node = (dev_ms - hash_ms) / dev_ms, info['device_bytes'] / info['nodes']
            rows['rows'][k] = dict(hashes=k * depth, update_ms=[s * 1e3 for s in upd], device_ms=dev_ms, hash_launches_ms=hash_ms, not_hashing_share=other,
                                   update_hashes_per_s=k * depth / upd[1], leaves=info['leaves'], nodes=info['nodes'], device_bytes=info['device_bytes'],
                                   bytes_per_node=per_node)
            print('sparse 2^%d  k %8d  %9d hashes  update %9.3f ms (%.4g hashes/s)  on the device %9.3f ms: hash launches %9.3f ms, not hashing %5.1f %%  '
                  '%.1f bytes per stored node' % (lg, k, k * depth, upd[1] * 1e3, k * depth / upd[1], dev_ms, hash_ms, 100 * other, per_node))
        tree.free()

    n = 1 << dd
    d_nodes = ctx.dev_alloc(32 * (2 * n - 1))
    ctx.gen_scalars_dev(d_nodes, n, 11)
    ctx.merkle_tree_dev(pp, d_nodes, n, d_nodes)
    for k in writes:
        ctx.upload(d_idx, rng.integers(0, n, k, dtype=np.uint64))
        upd, _ = timed(ctx, lambda: merkle.update_dev(ctx, pp, d_nodes, dd, d_idx, d_new, k, d_old, d_sib, d_roots), args.window, args.repeats)
        dev_ms, hash_ms = median_timed(lambda: merkle.update_timed_dev(ctx, pp, d_nodes, dd, d_idx, d_new, k, d_old, d_sib, d_roots), args.repeats)
        other = (dev_ms - hash_ms) / dev_ms
        res['dense'][k] = dict(hashes=k * dd, update_ms=[s * 1e3 for s in upd], device_ms=dev_ms, hash_launches_ms=hash_ms, not_hashing_share=other,
                               update_hashes_per_s=k * dd / upd[1], bytes_per_node=32.0)
        print('dense  2^%d  k %8d  %9d hashes  update %9.3f ms (%.4g hashes/s)  on the device %9.3f ms: hash launches %9.3f ms, not hashing %5.1f %%  '
              '32.0 bytes per node' % (dd, k, k * dd, upd[1] * 1e3, k * dd / upd[1], dev_ms, hash_ms, 100 * other))
    for d in (d_nodes, d_idx, d_new, d_old, d_sib, d_roots):
        ctx.dev_free(d)
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
