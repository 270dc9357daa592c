/* Bulk leaf writes to the Merkle trees on the device: the final state of an ordered update, one hash per touched node
 * (csrc/merkle_plan.hpp; the sparse tree's entries in csrc/sparse_merkle.hip, the dense tree's in csrc/merkle_update.hip).
 *
 * fk_smt_update* and fk_poseidon_merkle_update* apply k writes in list order and return a proof per write: every write walks its whole
 * path, k x depth hashes, which is what a rollup batch needs.  Loading a saved tree, applying a genesis allocation or following a
 * chain's state needs the final tree and its root alone.  The calls here take the same (index, leaf) list and leave the tree in EXACTLY
 * the state the ordered update of that list leaves it in -- for an index that occurs several times the write with the largest position
 * wins; a sparse tree stores the same nodes, every ancestor of a written index, a leaf written as 0 stored as 0 -- but hash every
 * distinct touched node once: 2^24 leaves at indices 0 .. 2^24 - 1 of a depth-32 tree are 16 777 223 hashes instead of 536 870 912.
 * There are no old leaves, no siblings and no per-write roots; the new root is the only output.
 *
 * Restoring a sparse tree: fk_smt_new, then ONE fk_smt_set of what fk_smt_export_level(0) of the saved tree gave.
 *
 * Cost: one stable sort of the writes by (index, position), then per level one launch that stores the level's distinct touched nodes,
 * one rocPRIM select that compacts their distinct parents, and one launch that hashes ONE PARENT PER LANE, the lanes dense.  The
 * counts of distinct nodes stay in device memory: nothing is downloaded between levels.
 *
 * Conventions: field elements are Montgomery limbs (4 x u64) as everywhere; k = 0 touches nothing.  Refusals (FK_ERR_BAD_ARG), all
 * before a byte of the tree or of an output is written: a null context, tree, index or leaf array (k > 0); a tree of another context;
 * k > 2^28 (FK_SMT_MAX_WRITES, FK_MERKLE_UPDATE_MAX_WRITES); an index that is not below 2^depth (found on the device, one flag
 * downloaded); for the dense tree parameters with t != 3 and depth > 40, as in fk_poseidon_merkle_update*.  A sparse table that must
 * grow and cannot is FK_ERR_OOM with the tree as it was.  Depth 0: the tree is its root, and the last write is the root.
 *
 * Scratch: the update's 92 bytes per write (two arrays of k node values; two of k node keys; the order, the identity and the selected
 * positions) and 8 (depth + 1) bytes of counts, plus rocPRIM's temporary storage, from the context's grow-only staging buffers.
 *
 * Declared here, not in fawkes_hip_sparse_merkle.h or fawkes_hip_merkle.h: each of those two describes one ctypes table, as
 * fawkes_hip.h does. */
#ifndef FAWKES_HIP_MERKLE_SET_H
#define FAWKES_HIP_MERKLE_SET_H
#include "fawkes_hip_merkle.h"
#include "fawkes_hip_sparse_merkle.h"
#ifdef __cplusplus
extern "C" {
#endif

/* sparse tree.  Everything but the index check (one flag is downloaded before the first write) and a growth of the tables is queued on
 * the context's stream: fk_sync, or a download, before d_root is read. */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_smt_set_dev(fk_ctx *ctx, fk_smt *tree, const void *d_indices /* k x u64 */, const void *d_leaves /* k x Fr */, size_t k,
                   void *d_root /* Fr or NULL */);
/* the same with the writes and the root in host memory; blocks */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_smt_set(fk_ctx *ctx, fk_smt *tree, const uint64_t *indices, const uint64_t *leaves, size_t k, uint64_t root[4] /* or NULL */);
/* measurement and test aid (tools/merkle_set_bench.py): fk_smt_set_dev, then a wait.  ms[0] = the whole call on the device (a growth
 * of the tables not included), ms[1] = its `depth` hash launches alone (HIP events around each); distinct[l], l = 0 .. depth = the
 * number of distinct touched nodes of level l, which is the number of lanes that stored (l < depth) and hashed (l > 0) there
 * (distinct[depth] = 1).  Either may be NULL */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_smt_set_timed_dev(fk_ctx *ctx, fk_smt *tree, const void *d_indices, const void *d_leaves, size_t k, void *d_root,
                         double ms[2], uint64_t *distinct /* depth + 1 */);

/* dense tree (fk_poseidon_merkle_tree_dev's layout: the root is the last node of d_nodes).  Queued like fk_smt_set_dev */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_poseidon_merkle_set_dev(fk_ctx *ctx, const fk_poseidon *params, void *d_nodes, uint32_t depth,
                               const void *d_indices /* k x u64 */, const void *d_leaves /* k x Fr */, size_t k);
/* the same with the writes in host memory; the tree stays resident; blocks */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_poseidon_merkle_set(fk_ctx *ctx, const fk_poseidon *params, void *d_nodes, uint32_t depth,
                           const uint64_t *indices, const uint64_t *leaves, size_t k);
/* measurement and test aid: fk_poseidon_merkle_set_dev, then a wait; ms and distinct as in fk_smt_set_timed_dev */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_poseidon_merkle_set_timed_dev(fk_ctx *ctx, const fk_poseidon *params, void *d_nodes, uint32_t depth,
                                     const void *d_indices, const void *d_leaves, size_t k, double ms[2], uint64_t *distinct /* depth + 1 */);

#ifdef __cplusplus
}
#endif
#endif
