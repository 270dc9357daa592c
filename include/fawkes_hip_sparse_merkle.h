/* Sparse Merkle state on the device: a Poseidon tree of depth up to 63 of which only the nodes ever written are stored
 * (csrc/sparse_merkle.hip).
 *
 * The dense tree of fawkes_hip_merkle.h holds 2^(depth + 1) - 1 nodes; at the depth of a rollup's account tree (32) that is 275 GB,
 * nearly all of it the hash of zeros.  A sparse tree stores, per level, the nodes some write has passed through, in an open-addressing
 * hash table in device memory (40 bytes per slot, load at most one half); a node that is not stored has the value zero[l] of its level,
 * zero[0] = 0, zero[l + 1] = H(zero[l], zero[l]) -- the value a dense tree gives its zero padding, so both agree on every root and
 * sibling.  Entries are never removed: a leaf written back to 0 stays stored with the value 0.
 *
 * fk_smt_update* is the contract of fk_poseidon_merkle_update*: k leaf writes applied IN THE ORDER GIVEN; for write j the leaf it
 * replaced, its depth siblings as of its own moment (siblings[j * depth + l], leaf level first) and the root after it.  One launch of k
 * hashes per level whatever the collisions among the indices.  fk_smt_proofs* reads: the stored (or default) leaf and siblings of any
 * index, nothing is changed.  fk_smt_export_level lists what a level stores; level 0 is how a tree is saved: a new tree given the
 * exported leaves has the same root -- through the bulk write of fawkes_hip_merkle_set.h, which hashes every node once and returns no
 * proofs (the ordered update here restores the same tree at depth hashes per leaf).
 *
 * Conventions: field elements are Montgomery limbs (4 x u64) as everywhere; any output may be NULL; k = 0 (n = 0) touches nothing.
 * Refusals (FK_ERR_BAD_ARG), all before a byte of the tree or of an output is written: parameters with t != 3; depth > FK_SMT_MAX_DEPTH;
 * k > FK_SMT_MAX_WRITES; a null tree, index or leaf array; a tree of another context; an index that is not below 2^depth (found on the
 * device, one flag downloaded).  A table that must grow and cannot is FK_ERR_OOM with the tree as it was.
 *
 * A tree belongs to the context that made it and is freed before it; fk_trim does not touch trees.  The update borrows the context's
 * staging buffers (92 bytes per write plus the sort's); the reading entries touch only the small `misc` buffer.
 *
 * Declared here, not in fawkes_hip.h: that header, its ctypes table and the Rust shim describe one pinned ABI; fawkes_hip_merkle.h is
 * the precedent. */
#ifndef FAWKES_HIP_SPARSE_MERKLE_H
#define FAWKES_HIP_SPARSE_MERKLE_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fk_smt fk_smt;
#define FK_SMT_MAX_DEPTH 63            /* a node index keeps one value (all ones) for "empty slot" */
#define FK_SMT_MIN_SLOTS 64            /* the smallest table of a level */
#define FK_SMT_MAX_WRITES ((size_t)1 << 28)   /* the position of a write in the list is kept in 32 bits */

/* an empty tree of 2^depth leaves, all 0: its root is zero[depth].  expected_leaves sizes the tables so that this many distinct leaves
 * fit without a growth (0: the smallest tables; they grow as needed).  Blocks (the defaults are hashed on the device) */
int fk_smt_new(fk_ctx *ctx, const fk_poseidon *params, uint32_t depth, uint64_t expected_leaves, fk_smt **out);
void fk_smt_free(fk_ctx *ctx, fk_smt *tree);
/* out: depth, stored leaves, stored nodes (all levels), device bytes.  Blocks */
int fk_smt_info(fk_ctx *ctx, const fk_smt *tree, uint64_t out[4]);
/* out: (depth + 1) x 4 limbs, zero[0 .. depth].  Host only */
int fk_smt_defaults(const fk_smt *tree, uint64_t *out);
/* blocks */
int fk_smt_root(fk_ctx *ctx, const fk_smt *tree, uint64_t root[4]);

/* apply k leaf writes IN ORDER; any of the three outputs may be NULL.  Everything but the index check (one flag is downloaded before the
 * first write) and a growth of the tables is queued on the context's stream: fk_sync, or a download, before the outputs are read. */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_smt_update_dev(fk_ctx *ctx, fk_smt *tree, const void *d_indices /* k x u64 */, const void *d_new_leaves /* k x Fr */, size_t k,
                      void *d_old_leaves /* k x Fr */, void *d_siblings /* k x depth x Fr */, void *d_roots /* k x Fr */);
/* the same with the writes and the outputs in host memory; blocks */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_smt_update(fk_ctx *ctx, fk_smt *tree, const uint64_t *indices, const uint64_t *new_leaves, size_t k,
                  uint64_t *old_leaves, uint64_t *siblings, uint64_t *roots);
/* measurement aid (tools/sparse_merkle_bench.py): fk_smt_update_dev, then a wait; ms[0] = the whole update on the device (a growth of
 * the tables not included), ms[1] = its `depth` hash launches alone (HIP events around each) */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_smt_update_timed_dev(fk_ctx *ctx, fk_smt *tree, const void *d_indices, const void *d_new_leaves, size_t k,
                            void *d_old_leaves, void *d_siblings, void *d_roots, double ms[2]);

/* read only: leaves[i] = the leaf at indices[i] (0 where none was written), siblings[i * depth + l] = its sibling at level l (zero[l]
 * where the subtree is untouched).  Either output may be NULL.  The _dev entry downloads one flag (the index check) and queues the rest */
int fk_smt_proofs_dev(fk_ctx *ctx, const fk_smt *tree, const void *d_indices /* n x u64 */, size_t n, void *d_leaves /* n x Fr */,
                      void *d_siblings /* n x depth x Fr */);
int fk_smt_proofs(fk_ctx *ctx, const fk_smt *tree, const uint64_t *indices, size_t n, uint64_t *leaves, uint64_t *siblings);
/* the stored entries of a level (0 = leaves .. depth = the root alone), ascending by key, zero-valued ones included: *n = how many;
 * keys (node indices at that level) and vals (4 limbs each) are filled when keys is not NULL, and then cap < *n is refused.  Blocks */
int fk_smt_export_level(fk_ctx *ctx, const fk_smt *tree, uint32_t level, uint64_t *keys, uint64_t *vals, size_t cap, size_t *n);

#ifdef __cplusplus
}
#endif
#endif
