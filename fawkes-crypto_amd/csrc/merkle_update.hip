// Ordered leaf writes to a resident Poseidon Merkle tree, with the proof of every write (include/fawkes_hip_merkle.h).
//
// Write j of k replaces leaf idx[j]; it must see the tree as the writes 0 .. j - 1 left it.  At level l the only thing write j needs
// from elsewhere is the value of its SIBLING node at its own moment: the value left there by the latest earlier write i < j that passes
// through that node (its "previous toucher"), or the stored node when there is none.  Neither depends on level l of write j itself, so
// a level is ONE launch of k independent hashes, and no chain of dependent hashes is longer than the depth.
//
// Who the previous toucher is depends on the indices alone.  The writes are sorted ONCE by (index, j) (a stable radix sort over the
// depth index bits of the pairs (index, j) in list order); at level l the order array is sorted by (index >> l, j), so the writes
// through one node form a contiguous run, ascending in j.  Per level:
//   plan        one write per lane, by position q in the order: binary searches on the node keys give the run of the lane's own node
//               [a, b) and of the sibling node [c, d) (the two are neighbours: they share the parent), a binary search on j inside the
//               sibling run gives r = its writes earlier than j; the previous toucher is element r - 1 of that run; the lane's position
//               in the next level's order is min(a, c) + (q - a) + r -- the two runs merged by rank, no second sort
//   hash        one write per lane, by j: sib = the previous toucher's current value or the stored node; next[j] = H(cur[j], sib) or
//               H(sib, cur[j]); sib goes to siblings[j * depth + l].  No search in this kernel: it keeps the register budget of the
//               t = 3 hash kernels
//   write-back  the last write of each run stores its current value into level l of the tree -- in a launch of its own BEHIND the hash
//               launch of that level: a write j whose sibling has no earlier toucher reads the STORED node there, and a later write
//               i > j through that sibling would otherwise overwrite it first
// After the last level cur[j] is the root after write j.  The old leaf of a write is the new leaf of the previous element of its run at
// level 0, or the stored leaf.
//
// Scratch per call (documented in the header): cur / next (2 k Fr, ctx->stage_a); keys, next keys (k u64 each), order, next order,
// previous touchers (k u32 each) (ctx->stage_b); the sort's temporary storage (ctx->stage_c).  This sort, the same one in sparse_merkle.hip and the bulk write's
// select (merkle_plan.hpp) are the library's use of rocPRIM.
//
// Set of k writes (include/fawkes_hip_merkle_set.h: the final tree of the update and nothing else): merkle_plan.hpp's bulk write with
// the node array as the store of a level -- put is a plain store, get the address of the node.  The write-back of a level is a launch
// of its own in front of the level's hash launch (the shared driver's order): a node is either written or read as an absent child,
// never both, so the hash launch reads nodes that no launch beside it writes.
#include "merkle_plan.hpp"      // the index check, the plan kernel, the bulk write and the drivers' small helpers: shared with sparse_merkle.hip
#include "../../include/fawkes_hip_merkle.h"
#include "../../include/fawkes_hip_merkle_set.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace fk {

// level 0 only: what each write replaces.  keys / ord: the level-0 order
__global__ __launch_bounds__(POS_THREADS) void mu_old_leaves_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ord, uint32_t k,
                                                                     const Fr *__restrict__ leaves, const Fr *__restrict__ new_leaves, Fr *__restrict__ old) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t node = keys[q];
    old[ord[q]] = (q > 0 && keys[q - 1] == node) ? new_leaves[ord[q - 1]] : leaves[node];
}

// level: the stored nodes of level l; cur: the writes' values at level l (by j); sib_out: siblings + l, or null
__global__ __launch_bounds__(POS_THREADS) void mu_hash_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr *__restrict__ level,
                                                               const uint64_t *__restrict__ idx, uint32_t l, uint32_t depth, const uint32_t *__restrict__ prev,
                                                               const Fr *__restrict__ cur, uint32_t k, Fr *__restrict__ next, Fr *__restrict__ sib_out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint64_t node = idx[j] >> l;
    const uint32_t pj = prev[j];
    const Fr sib = pj != MU_NONE ? cur[pj] : level[node ^ 1];
    const Fr own = cur[j];
    if (sib_out) sib_out[(size_t)j * depth] = sib;
    const bool right = node & 1;
    Fr x, y;
#pragma unroll
    for (int i = 0; i < 8; i++) { x.v[i] = right ? sib.v[i] : own.v[i]; y.v[i] = right ? own.v[i] : sib.v[i]; }
    next[j] = hash2(tab, f, p, x, y);
}

// the last write of each run leaves its value in the tree
__global__ __launch_bounds__(POS_THREADS) void mu_write_back_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ord, uint32_t k,
                                                                     const Fr *__restrict__ cur, Fr *__restrict__ level) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t node = keys[q];
    if (q + 1 == k || keys[q + 1] != node) level[node] = cur[ord[q]];
}

static int update_args(fk_ctx *ctx, const fk_poseidon *h, uint32_t depth, size_t k) {
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (h->t != 3) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: the tree hashes pairs with t = 3 parameters (got t = %u)", h->t);
    if (depth > POS_MAX_TREE_DEPTH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: depth %u is larger than any tree in device memory (max %u)", depth, POS_MAX_TREE_DEPTH);
    if (k > FK_MERKLE_UPDATE_MAX_WRITES) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: one update takes at most 2^28 writes (got %zu)", k);
    return FK_OK;
}

// k >= 1, arguments checked.  ms: null, or where the timed entry wants the device times (then the call waits for the stream)
static int update_dev(fk_ctx *ctx, const fk_poseidon *h, Fr *d_nodes, uint32_t depth, const uint64_t *d_idx, const Fr *d_new, uint32_t k, Fr *d_old, Fr *d_sib,
                      Fr *d_roots, double *ms) {
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
    const dim3 grid(pos_blocks(k)), block(POS_THREADS);
    // the indices first: nothing is written before they are known to be good
    FK_HIP(ctx, hipMemsetAsync(d.flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(mu_check_kernel, grid, block, 0, ctx->stream, d_idx, k, depth, d.flag);
    FK_HIP(ctx, hipGetLastError());
    uint32_t bad = 0;
    FK_HIP(ctx, hipMemcpyAsync(&bad, d.flag, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: a leaf index of the update is not below 2^%u (nothing was written: the tree and the outputs are as they were)", depth);

    size_t sort_bytes = 0;
    uint64_t *keys = nullptr, *next_keys = nullptr;
    uint32_t *ord = nullptr, *next_ord = nullptr, *prev = nullptr;
    if (depth) FK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, d_idx, keys, (const uint32_t *)next_ord, ord, (size_t)k, 0u, depth, ctx->stream));
    FK_HIP(ctx, ctx->stage_a.reserve((size_t)2 * k * sizeof(Fr)));
    FK_HIP(ctx, ctx->stage_b.reserve((size_t)k * (2 * sizeof(uint64_t) + 3 * sizeof(uint32_t))));
    FK_HIP(ctx, ctx->stage_c.reserve(sort_bytes ? sort_bytes : 8));
    Fr *val[2] = {ctx->stage_a.as<Fr>(), ctx->stage_a.as<Fr>() + k};
    keys = ctx->stage_b.as<uint64_t>(); next_keys = keys + k;
    ord = (uint32_t *)(next_keys + k); next_ord = ord + k; prev = next_ord + k;

    MuEvents tm;
    if (ms) { FK_HIP(ctx, tm.make(2 + 2 * (size_t)depth)); FK_HIP(ctx, hipEventRecord(tm.ev[0], ctx->stream)); }

    // the level-0 order: a stable sort of (index, j) by the index
    if (depth) {
        hipLaunchKernelGGL(mu_iota_kernel, grid, block, 0, ctx->stream, next_ord, k);
        FK_HIP(ctx, hipGetLastError());
        FK_HIP(ctx, rocprim::radix_sort_pairs(ctx->stage_c.p, sort_bytes, d_idx, keys, (const uint32_t *)next_ord, ord, (size_t)k, 0u, depth, ctx->stream));
    } else {
        hipLaunchKernelGGL(mu_iota_kernel, grid, block, 0, ctx->stream, ord, k);
        FK_HIP(ctx, hipMemsetAsync(keys, 0, (size_t)k * sizeof(uint64_t), ctx->stream));
    }
    if (d_old) hipLaunchKernelGGL(mu_old_leaves_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys, (const uint32_t *)ord, k, (const Fr *)d_nodes, d_new, d_old);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "merkle update: sort");

    const Fr *cur = d_new;
    Fr *level = d_nodes;
    for (uint32_t l = 0; l < depth; l++) {
        Fr *next = val[l & 1];
        hipLaunchKernelGGL(mu_plan_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys, (const uint32_t *)ord, k, prev, next_keys, next_ord);
        if (ms) FK_HIP(ctx, hipEventRecord(tm.ev[2 + 2 * l], ctx->stream));
        hipLaunchKernelGGL(mu_hash_kernel, grid, block, 0, ctx->stream, d.tab, h->f, h->p, (const Fr *)level, d_idx, l, depth, (const uint32_t *)prev, cur, k, next,
                           d_sib ? d_sib + l : (Fr *)nullptr);
        if (ms) FK_HIP(ctx, hipEventRecord(tm.ev[3 + 2 * l], ctx->stream));
        hipLaunchKernelGGL(mu_write_back_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys, (const uint32_t *)ord, k, cur, level);
        FK_HIP(ctx, hipGetLastError());
        FK_DBG(ctx, "merkle update: level");
        std::swap(keys, next_keys); std::swap(ord, next_ord);
        cur = next;
        level += (uint64_t)1 << (depth - l);
    }
    // every write passes through the root: the last of the list leaves its value there
    if (d_roots) FK_HIP(ctx, hipMemcpyAsync(d_roots, cur, (size_t)k * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(level, cur + (k - 1), sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (ms) {
        FK_HIP(ctx, hipEventRecord(tm.ev[1], ctx->stream));
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float t = 0;
        FK_HIP(ctx, hipEventElapsedTime(&t, tm.ev[0], tm.ev[1]));
        ms[0] = t; ms[1] = 0;
        for (uint32_t l = 0; l < depth; l++) { FK_HIP(ctx, hipEventElapsedTime(&t, tm.ev[2 + 2 * l], tm.ev[3 + 2 * l])); ms[1] += t; }
    }
    return FK_OK;
}

// a level as merkle_plan.hpp's bulk write sees it
struct DenseStore {
    Fr *level;
    __device__ __forceinline__ void put(uint64_t key, const Fr &v) const { level[key] = v; }
    __device__ __forceinline__ const Fr *get(uint64_t key) const { return level + key; }
};

// k >= 1, arguments checked, the staging claimed.  timed: null, or what the timed entry wants (then the call waits for the stream)
static int set_dev(fk_ctx *ctx, const fk_poseidon *h, Fr *d_nodes, uint32_t depth, const uint64_t *d_idx, const Fr *d_leaves, uint32_t k, const MsTimed *timed) {
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
    FK_TRY(ms_check_indices(ctx, d.flag, d_idx, k, depth, "merkle"));
    if (depth == 0) return ms_set_depth0(ctx, d_leaves, k, d_nodes, nullptr, timed);
    MsScratch s; FK_TRY(ms_reserve(ctx, d_idx, depth, k, &s));
    MuEvents tm;
    if (timed) FK_HIP(ctx, tm.make(2 + 2 * (size_t)depth));
    // level l begins behind the 2^depth + .. + 2^(depth - l + 1) nodes of the levels below it; the root is the last node
    auto store_at = [&](uint32_t l) { return DenseStore{d_nodes + (((uint64_t)2 << depth) - ((uint64_t)2 << (depth - l)))}; };
    FK_TRY(ms_set_levels(ctx, d.tab, h->f, h->p, depth, d_idx, d_leaves, k, s, store_at, d_nodes + (((uint64_t)2 << depth) - 2), (Fr *)nullptr, timed ? &tm : nullptr));
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
    // one block: new leaves | old leaves | roots | siblings | indices (the outputs are used only where asked for)
    const size_t ib = k * sizeof(uint64_t), lb = k * sizeof(Fr), sb = siblings ? lb * depth : 0;
    MuDevBlock blk;
    FK_HIP(ctx, hipMalloc(&blk.p, 3 * lb + sb + ib));
    Fr *d_new = (Fr *)blk.p, *d_old = old_leaves ? d_new + k : nullptr, *d_roots = roots ? d_new + 2 * k : nullptr, *d_sib = sb ? d_new + 3 * k : nullptr;
    uint64_t *d_idx = (uint64_t *)((uint8_t *)blk.p + 3 * lb + sb);
    FK_HIP(ctx, hipMemcpyAsync(d_idx, indices, ib, hipMemcpyHostToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(d_new, new_leaves, lb, hipMemcpyHostToDevice, ctx->stream));
    int rc = update_dev(ctx, h, (Fr *)d_nodes, depth, d_idx, d_new, (uint32_t)k, d_old, d_sib, d_roots, nullptr);
    if (rc == FK_OK) {
        auto down = [&]() -> int {
            if (d_old) FK_HIP(ctx, hipMemcpyAsync(old_leaves, d_old, lb, hipMemcpyDeviceToHost, ctx->stream));
            if (d_roots) FK_HIP(ctx, hipMemcpyAsync(roots, d_roots, lb, hipMemcpyDeviceToHost, ctx->stream));
            if (d_sib) FK_HIP(ctx, hipMemcpyAsync(siblings, d_sib, sb, hipMemcpyDeviceToHost, ctx->stream));
            return FK_OK;
        };
        rc = down();
    }
    (void)hipStreamSynchronize(ctx->stream);      // the block is in use until the stream has drained, on the error paths too
    return rc;
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
    // one block: leaves | indices
    const size_t ib = k * sizeof(uint64_t), lb = k * sizeof(Fr);
    MuDevBlock blk;
    FK_HIP(ctx, hipMalloc(&blk.p, lb + ib));
    Fr *d_leaves = (Fr *)blk.p;
    uint64_t *d_idx = (uint64_t *)(d_leaves + k);
    FK_HIP(ctx, hipMemcpyAsync(d_idx, indices, ib, hipMemcpyHostToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(d_leaves, leaves, lb, hipMemcpyHostToDevice, ctx->stream));
    const int rc = set_dev(ctx, h, (Fr *)d_nodes, depth, d_idx, d_leaves, (uint32_t)k, nullptr);
    (void)hipStreamSynchronize(ctx->stream);      // the block is in use until the stream has drained, on the error paths too
    return rc;
}); }

}  // extern "C"
