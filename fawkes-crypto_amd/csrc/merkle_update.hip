// Resident dense Poseidon Merkle trees (include/fawkes_hip_merkle.h, include/fawkes_hip_merkle_set.h): ordered leaf writes with the
// proof of every write, and the bulk write that leaves the same tree and nothing else.
//
// Both are merkle_plan.hpp's drivers (the scheme, the kernels and the scratch are described there) with the node array as the store of
// a level: put is a plain store, get the address of the node.  What is here: the store, the argument checks and the extern "C" entries.
// The update's write-back follows the hash launch of its level and the set's precedes it -- the shared drivers' orders, and in both the
// hash launch reads nodes that no launch beside it writes.
#include "merkle_plan.hpp"
#include "../../include/fawkes_hip_merkle.h"
#include "../../include/fawkes_hip_merkle_set.h"

namespace fk {

// a level as merkle_plan.hpp's drivers see it
struct DenseStore {
    Fr *level;
    __device__ __forceinline__ void put(uint64_t key, const Fr &v) const { level[key] = v; }
    __device__ __forceinline__ const Fr *get(uint64_t key) const { return level + key; }
};
// level l begins behind the 2^depth + .. + 2^(depth - l + 1) nodes of the levels below it; the root (l = depth) is the last node
static inline Fr *dense_level(Fr *d_nodes, uint32_t depth, uint32_t l) { return d_nodes + (((uint64_t)2 << depth) - ((uint64_t)2 << (depth - l))); }

static int update_args(fk_ctx *ctx, const fk_poseidon *h, uint32_t depth, size_t k) {
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (h->t != 3) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: the tree hashes pairs with t = 3 parameters (got t = %u)", h->t);
    if (depth > POS_MAX_TREE_DEPTH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: depth %u is larger than any tree in device memory (max %u)", depth, POS_MAX_TREE_DEPTH);
    if (k > FK_MERKLE_UPDATE_MAX_WRITES) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: one update takes at most 2^28 writes (got %zu)", k);
    return FK_OK;
}

// k >= 1, arguments checked, the staging claimed.  ms: null, or where the timed entry wants the device times (then the call waits for the stream)
static int update_dev(fk_ctx *ctx, const fk_poseidon *h, Fr *d_nodes, uint32_t depth, const uint64_t *d_idx, const Fr *d_new, uint32_t k, Fr *d_old, Fr *d_sib,
                      Fr *d_roots, double *ms) {
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
    // the indices first: nothing is written before they are known to be good
    FK_TRY(ms_check_indices(ctx, d.flag, d_idx, k, depth, "merkle", "update", MU_UPDATE_TAIL));
    if (depth == 0) return mu_update_depth0(ctx, d_new, k, d_nodes, d_old, d_roots, ms);
    MuScratch s; FK_TRY(mu_reserve(ctx, d_idx, depth, k, &s));
    MuEvents tm;
    if (ms) FK_HIP(ctx, tm.make(2 + 2 * (size_t)depth));
    auto store_at = [&](uint32_t l) { return DenseStore{dense_level(d_nodes, depth, l)}; };
    FK_TRY(mu_update_levels(ctx, d.tab, h->f, h->p, depth, d_idx, d_new, k, s, store_at, dense_level(d_nodes, depth, depth), d_old, d_sib, d_roots, ms ? &tm : nullptr));
    return ms ? mu_finish_timed(ctx, tm, depth, ms) : FK_OK;
}

// k >= 1, arguments checked, the staging claimed.  timed: null, or what the timed entry wants (then the call waits for the stream)
static int set_dev(fk_ctx *ctx, const fk_poseidon *h, Fr *d_nodes, uint32_t depth, const uint64_t *d_idx, const Fr *d_leaves, uint32_t k, const MsTimed *timed) {
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
    FK_TRY(ms_check_indices(ctx, d.flag, d_idx, k, depth, "merkle", "set", MS_SET_TAIL));
    if (depth == 0) return ms_set_depth0(ctx, d_leaves, k, d_nodes, nullptr, timed);
    MsScratch s; FK_TRY(ms_reserve(ctx, d_idx, depth, k, &s));
    MuEvents tm;
    if (timed) FK_HIP(ctx, tm.make(2 + 2 * (size_t)depth));
    auto store_at = [&](uint32_t l) { return DenseStore{dense_level(d_nodes, depth, l)}; };
    FK_TRY(ms_set_levels(ctx, d.tab, h->f, h->p, depth, d_idx, d_leaves, k, s, store_at, dense_level(d_nodes, depth, depth), (Fr *)nullptr, timed ? &tm : nullptr));
    if (timed) FK_TRY(ms_finish_timed(ctx, tm, depth, s, *timed));
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_poseidon_merkle_update_timed_dev(fk_ctx *ctx, const fk_poseidon *h, void *d_nodes, uint32_t depth, const void *d_indices, const void *d_new_leaves, size_t k,
                                        void *d_old_leaves, void *d_siblings, void *d_roots, double ms[2]) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(update_args(ctx, h, depth, k));
    if (ms) ms[0] = ms[1] = 0;
    if (!k) return FK_OK;
    if (!d_nodes || !d_indices || !d_new_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "merkle update"));      // update_dev sorts in stage_a/b/c
    return update_dev(ctx, h, (Fr *)d_nodes, depth, (const uint64_t *)d_indices, (const Fr *)d_new_leaves, (uint32_t)k, (Fr *)d_old_leaves, (Fr *)d_siblings,
                      (Fr *)d_roots, ms);
}); }

int fk_poseidon_merkle_update_dev(fk_ctx *ctx, const fk_poseidon *h, void *d_nodes, uint32_t depth, const void *d_indices, const void *d_new_leaves, size_t k,
                                  void *d_old_leaves, void *d_siblings, void *d_roots) {
    return fk_poseidon_merkle_update_timed_dev(ctx, h, d_nodes, depth, d_indices, d_new_leaves, k, d_old_leaves, d_siblings, d_roots, nullptr);
}

int fk_poseidon_merkle_update(fk_ctx *ctx, const fk_poseidon *h, void *d_nodes, uint32_t depth, const uint64_t *indices, const uint64_t *new_leaves, size_t k,
                              uint64_t *old_leaves, uint64_t *siblings, uint64_t *roots) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(update_args(ctx, h, depth, k));
    if (!k) return FK_OK;
    if (!d_nodes || !indices || !new_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "merkle update"));
    MuArray a[] = {{new_leaves, nullptr, k}, {nullptr, old_leaves, k}, {nullptr, roots, k}, {nullptr, siblings, k * depth}};
    return mu_host_call(ctx, indices, k, a, [&](const uint64_t *d_idx) {
        return update_dev(ctx, h, (Fr *)d_nodes, depth, d_idx, a[0].d, (uint32_t)k, a[1].d, a[3].d, a[2].d, nullptr);
    });
}); }

// ---- include/fawkes_hip_merkle_set.h
int fk_poseidon_merkle_set_timed_dev(fk_ctx *ctx, const fk_poseidon *h, void *d_nodes, uint32_t depth, const void *d_indices, const void *d_leaves, size_t k,
                                     double ms[2], uint64_t *distinct) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(update_args(ctx, h, depth, k));
    if (ms) ms[0] = ms[1] = 0;
    if (!k) return FK_OK;
    if (!d_nodes || !d_indices || !d_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "merkle set"));      // merkle_plan.hpp's bulk write sorts and selects in stage_a/b/c
    const MsTimed timed{ms, distinct};
    return set_dev(ctx, h, (Fr *)d_nodes, depth, (const uint64_t *)d_indices, (const Fr *)d_leaves, (uint32_t)k, &timed);
}); }

int fk_poseidon_merkle_set_dev(fk_ctx *ctx, const fk_poseidon *h, void *d_nodes, uint32_t depth, const void *d_indices, const void *d_leaves, size_t k) {
    return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(update_args(ctx, h, depth, k));
    if (!k) return FK_OK;
    if (!d_nodes || !d_indices || !d_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "merkle set"));
    return set_dev(ctx, h, (Fr *)d_nodes, depth, (const uint64_t *)d_indices, (const Fr *)d_leaves, (uint32_t)k, nullptr);
}); }

int fk_poseidon_merkle_set(fk_ctx *ctx, const fk_poseidon *h, void *d_nodes, uint32_t depth, const uint64_t *indices, const uint64_t *leaves, size_t k) {
    return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(update_args(ctx, h, depth, k));
    if (!k) return FK_OK;
    if (!d_nodes || !indices || !leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "merkle set"));
    MuArray a[] = {{leaves, nullptr, k}};
    return mu_host_call(ctx, indices, k, a, [&](const uint64_t *d_idx) { return set_dev(ctx, h, (Fr *)d_nodes, depth, d_idx, a[0].d, (uint32_t)k, nullptr); });
}); }

}  // extern "C"
