#!/usr/bin/env python3
"""Ordered leaf writes to a resident Merkle tree (csrc/merkle_update.hip), t = 3 parameters (3, 8, 53): a depth-24 tree and k uniform
random writes, k in {1741, 2^14, 2^20}.  Per k:
  update     fk_poseidon_merkle_update_dev with all three outputs (old leaves, siblings, roots)
  hashes     its `depth` hash launches alone (fk_poseidon_merkle_update_timed_dev: HIP events around each launch), and what is left of
             the update's device time -- the index check, the sort, the plans, the write-backs, the copies -- as a share of it
  batch      fk_poseidon_hash_batch_dev over k * depth pairs: the same number of hashes with nothing else
  rebuild    fk_poseidon_merkle_tree_dev over the 2^24 leaves: what a caller without the update would run (2^24 - 1 hashes)
`update`, `batch` and `rebuild` are host clocks around a stream synchronise, after a warm-up, over a window of at least --window seconds,
repeated --repeats times (median printed, min and max kept in the JSON); `hashes` is the median of --repeats timed calls.  The last line
is one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fawkes_crypto_amd as fk  # noqa: E402
from fawkes_crypto_amd import merkle  # noqa: E402
from poseidon_bench import timed  # noqa: E402

T, F, P = 3, 8, 53


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--writes', default='1741,16384,1048576')
    args = ap.parse_args()
    depth, n = args.depth, 1 << args.depth
    ctx = fk.Context(0)
    pp = fk.PoseidonParams(T, F, P)
    res = dict(depth=depth, window_s=args.window, repeats=args.repeats, rows={})
    d_nodes = ctx.dev_alloc(32 * (2 * n - 1))
    ctx.gen_scalars_dev(d_nodes, n, 11)
    secs, _ = timed(ctx, lambda: ctx.merkle_tree_dev(pp, d_nodes, n, d_nodes), args.window, args.repeats)
    res['rebuild_ms'] = [s * 1e3 for s in secs]
    print('library %s   depth %d   rebuild of the whole tree (%d hashes): %.3f ms' % (os.path.basename(fk.lib_path()), depth, n - 1, secs[1] * 1e3))
    rng = np.random.default_rng(24)
    for k in [int(x) for x in args.writes.split(',')]:
        d_idx, d_new, d_old, d_sib, d_roots = (ctx.dev_alloc(b) for b in (8 * k, 32 * k, 32 * k, 32 * k * depth, 32 * k))
        d_pairs, d_out = ctx.dev_alloc(64 * k * depth), ctx.dev_alloc(32 * k * depth)
        ctx.upload(d_idx, rng.integers(0, n, k, dtype=np.uint64))
        ctx.gen_scalars_dev(d_new, k, 13)
        ctx.gen_scalars_dev(d_pairs, 2 * k * depth, 17)
        upd, _ = timed(ctx, lambda: merkle.update_dev(ctx, pp, d_nodes, depth, d_idx, d_new, k, d_old, d_sib, d_roots), args.window, args.repeats)
        ev = sorted(merkle.update_timed_dev(ctx, pp, d_nodes, depth, d_idx, d_new, k, d_old, d_sib, d_roots) for _ in range(args.repeats))
        dev_ms, hash_ms = ev[len(ev) // 2]
        bat, _ = timed(ctx, lambda: ctx.poseidon_dev(pp, d_pairs, 2, k * depth, d_out), args.window, args.repeats)
        other = (dev_ms - hash_ms) / dev_ms
        res['rows'][k] = dict(hashes=k * depth, update_ms=[s * 1e3 for s in upd], device_ms=dev_ms, hash_launches_ms=hash_ms, not_hashing_share=other,
                              batch_ms=[s * 1e3 for s in bat], update_hashes_per_s=k * depth / upd[1], rebuild_over_update=secs[1] / upd[1])
        print('k %8d  %9d hashes  update %9.3f ms (%.4g hashes/s)  on the device %9.3f ms: hash launches %9.3f ms, not hashing %5.1f %%  '
              'hash batch %9.3f ms  rebuild / update %.2f' % (k, k * depth, upd[1] * 1e3, k * depth / upd[1], dev_ms, hash_ms, 100 * other, bat[1] * 1e3,
                                                              secs[1] / upd[1]))
        for d in (d_idx, d_new, d_old, d_sib, d_roots, d_pairs, d_out):
            ctx.dev_free(d)
    ctx.dev_free(d_nodes)
    print(json.dumps(res))
    ctx.close()


if __name__ == '__main__':
    main()
