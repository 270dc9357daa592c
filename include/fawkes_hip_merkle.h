/* Merkle state on the device: ordered leaf writes to a resident Poseidon tree, with one proof per write (csrc/merkle_update.hip).
 *
 * A rollup batch chains: transaction j + 1 starts from the root transaction j left, and the sibling path of transaction j is the path
 * in the tree as the transactions 0 .. j - 1 left it.  These calls take a tree built by fk_poseidon_merkle_tree_dev (levels one behind
 * the other, leaves first, root last, 2^(depth + 1) - 1 nodes) and k leaf writes, apply the writes IN THE ORDER GIVEN, and return for
 * write j the leaf it replaced, its depth siblings as of its own moment (siblings[j * depth + l], leaf level first: the layout of
 * fk_poseidon_merkle_proofs_dev, so the output feeds fk_poseidon_merkle_proof_roots_dev and the given rows of a witness program as it
 * is) and the root after it.  The tree is left in its final state.  The root before write j is roots[j - 1], or the stored root for
 * j = 0.  A write to the zero padding above n_leaves is an ordinary write: this is how a leaf is appended.
 *
 * Cost: one launch of k hashes per level, depth launches in all, whatever the collisions among the indices (k writes to one leaf are
 * as parallel as k writes to k leaves); one stable sort of the writes by (index, position); no download between levels.
 *
 * Refusals (FK_ERR_BAD_ARG), all before a byte of the tree or of an output is written: parameters with t != 3; depth > 40;
 * k > FK_MERKLE_UPDATE_MAX_WRITES; a null tree, index or leaf array; an index that is not below 2^depth.  k = 0 touches nothing.
 *
 * Scratch: 92 bytes per write (two arrays of k current values; the order, the next order, the node keys, the next node keys and the
 * previous-toucher indices) plus the sort's temporary storage (about 13 bytes per write), taken from the context's grow-only staging
 * buffers (fk_trim returns them); the host-memory call allocates device copies of its arguments and outputs and frees them on every
 * path, the error paths included.
 *
 * Declared here, not in fawkes_hip.h: that header, its ctypes table and the Rust shim describe one pinned ABI; fawkes_hip_witness.h,
 * fawkes_hip_verify.h and fawkes_hip_check.h are the precedent. */
#ifndef FAWKES_HIP_MERKLE_H
#define FAWKES_HIP_MERKLE_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FK_MERKLE_UPDATE_MAX_WRITES ((size_t)1 << 28)   /* the position of a write in the list is kept in 32 bits */

/* apply k leaf writes IN ORDER to a resident tree; any of the three outputs may be NULL.  Everything but the index check (one flag is
 * downloaded before the first write) is queued on the context's stream: fk_sync, or a download, before the outputs are read. */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_poseidon_merkle_update_dev(fk_ctx *ctx, const fk_poseidon *params, void *d_nodes, uint32_t depth,
                                  const void *d_indices /* k x u64 */, const void *d_new_leaves /* k x Fr */, size_t k,
                                  void *d_old_leaves /* k x Fr */, void *d_siblings /* k x depth x Fr */, void *d_roots /* k x Fr */);
/* the same with the writes and the outputs in host memory (Montgomery limbs, as everywhere); the tree stays resident; blocks */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_poseidon_merkle_update(fk_ctx *ctx, const fk_poseidon *params, void *d_nodes, uint32_t depth,
                              const uint64_t *indices, const uint64_t *new_leaves, size_t k,
                              uint64_t *old_leaves, uint64_t *siblings, uint64_t *roots);
/* measurement aid (tools/merkle_update_bench.py): fk_poseidon_merkle_update_dev, then a wait; ms[0] = the whole update on the device,
 * ms[1] = its `depth` hash launches alone (HIP events around each) */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_poseidon_merkle_update_timed_dev(fk_ctx *ctx, const fk_poseidon *params, void *d_nodes, uint32_t depth,
                                        const void *d_indices, const void *d_new_leaves, size_t k,
                                        void *d_old_leaves, void *d_siblings, void *d_roots, double ms[2]);

#ifdef __cplusplus
}
#endif
#endif
