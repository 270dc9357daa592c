// A sparse Poseidon Merkle tree resident in device memory: depth up to 63, only the nodes ever written are stored
// (include/fawkes_hip_sparse_merkle.h).
//
// Storage.  Level l = 0 .. depth - 1 (0 = leaves) has one open-addressing hash table: keys[cap] (u64, the node's index at its level;
// all ones = empty: an index is below 2^63) and vals[cap] (Fr), cap a power of two, linear probing from the top log2(cap) bits of
// key * 2^64 / phi (node indices come in runs: the multiplier spreads them), load at most one half.  A node that is not stored has the
// value zero[l].  The root is one Fr of its own.  Entries are never removed, so a probe that meets an empty slot has seen every slot its
// key could be in, and an insertion is one compare-and-swap on a key slot: no lane ever waits for another.
//
// Update of k ordered writes and set of k writes (the final state of the update, the new root and nothing else): merkle_plan.hpp's two
// drivers with this file's store of a level (SmtStore).  get is a bounded probe of the level's table that falls back to zero[l]; put
// claims the key's slot -- atomicCAS on a key slot, atomicAdd on the level's counter when it was empty -- and then stores the value
// plainly: the keys of one write-back launch are distinct.  In both drivers the write-back is a launch of its own beside the level's hash
// launch (behind it in the update, whose hash launch must read the stored sibling; in front of it in the set), so no probe ever runs
// beside a claim.  For the set the fused form would be sound -- a node is either in the list or read as an absent child, so a probe
// never looks for a key that a claim of the same launch inserts, and a claimed slot it walks over holds another key whenever it is read
// -- but it would save one latency-shaped launch per level and put the claim's registers into the hash kernel; the separate launch
// needs no argument at all.
//
// Capacity is settled BEFORE the first launch that writes: a call adds at most min(k, 2^(depth - l)) entries to level l; where the
// count's upper bound plus that exceeds cap / 2 a larger table is allocated (all of them first: a failure is FK_ERR_OOM with the tree as
// it was) and the old one rehashed into it, one lane per old slot, out of place.  The exact counts and the error word come to the host
// by ONE small download queued at the end of each update or set into pinned memory behind an event; the next call takes them when they
// have arrived and waits for them only if its upper bounds would otherwise force a growth.  Nothing is downloaded between levels.
// Every probe loop is bounded by the capacity; one that runs out (by construction none does) sets the error word and stops its lane.
#include "merkle_plan.hpp"
#include "../../include/fawkes_hip_sparse_merkle.h"
#include "../../include/fawkes_hip_merkle_set.h"
#include <algorithm>

struct fk_smt {
    fk_ctx *ctx = nullptr;
    uint32_t depth = 0;
    fk_poseidon h;                       // the tree's own copy of the parameters
    std::vector<fk::Fr> zero;            // zero[0 .. depth]
    // one device block: the Poseidon table | zero[0 .. depth] | the root | META_WORDS u64: the stored entries of level l at [l], the error word at [META_ERR]
    void *d_block = nullptr; size_t block_bytes = 0;
    fk::Fr *d_tab = nullptr, *d_zero = nullptr, *d_root = nullptr;
    unsigned long long *d_meta = nullptr;
    uint64_t *h_meta = nullptr;          // pinned: where the counts land
    hipEvent_t ev = nullptr;
    bool pending = false;                // a download of the counts is queued and has not been taken
    bool broken = false;                 // a probe ran out: the tables are not to be trusted
    struct Level { uint64_t *keys = nullptr; fk::Fr *vals = nullptr; uint32_t log_cap = 0; uint64_t count = 0, bound = 0; } lv[FK_SMT_MAX_DEPTH];
    // count: exact as of the last download taken; bound: count + what the updates queued since may have added
};

namespace fk {

static constexpr uint64_t SMT_EMPTY = ~(uint64_t)0, SMT_NOT_FOUND = ~(uint64_t)0;
static constexpr uint32_t SMT_META_WORDS = 64, SMT_META_ERR = 63;
static constexpr uint32_t SMT_MIN_LOG = 6;
static_assert((1u << SMT_MIN_LOG) == FK_SMT_MIN_SLOTS && FK_SMT_MAX_DEPTH <= SMT_META_ERR, "meta layout");

struct SmtTable { const uint64_t *keys; const Fr *vals; uint32_t log_cap; };
struct SmtTables { SmtTable t[FK_SMT_MAX_DEPTH]; };     // by value into the reading kernels (1.5 KB)

static __device__ __forceinline__ uint64_t smt_home(uint64_t key, uint32_t log_cap) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - log_cap); }

// the slot that holds `key`, or SMT_NOT_FOUND.  At most cap probes
static __device__ __forceinline__ uint64_t smt_find(const uint64_t *__restrict__ keys, uint32_t log_cap, uint64_t key, unsigned long long *err) {
    const uint64_t mask = ((uint64_t)1 << log_cap) - 1;
    uint64_t s = smt_home(key, log_cap);
    for (uint64_t n = 0; n <= mask; n++, s = (s + 1) & mask) {
        const uint64_t have = keys[s];
        if (have == key) return s;
        if (have == SMT_EMPTY) return SMT_NOT_FOUND;
    }
    atomicOr(err, 1ull);        // a full table: the capacity rule keeps the load at or below one half
    return SMT_NOT_FOUND;
}

// the slot of `key`, claimed if it was not there (then *count grows by one), or SMT_NOT_FOUND with the error word set.  At most cap probes
static __device__ __forceinline__ uint64_t smt_claim(uint64_t *__restrict__ keys, uint32_t log_cap, uint64_t key, unsigned long long *count, unsigned long long *err) {
    const uint64_t mask = ((uint64_t)1 << log_cap) - 1;
    uint64_t s = smt_home(key, log_cap);
    for (uint64_t n = 0; n <= mask; n++, s = (s + 1) & mask) {
        uint64_t have = keys[s];
        if (have == SMT_EMPTY) {
            have = atomicCAS((unsigned long long *)&keys[s], (unsigned long long)SMT_EMPTY, (unsigned long long)key);
            if (have == SMT_EMPTY) { if (count) atomicAdd(count, 1ull); return s; }
        }
        if (have == key) return s;
    }
    atomicOr(err, 2ull);
    return SMT_NOT_FOUND;
}

// zero[0] = 0, zero[l + 1] = H(zero[l], zero[l]): one lane, depth hashes in sequence (once per tree)
__global__ void smt_defaults_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, uint32_t depth, Fr *__restrict__ zero) {
    if (blockIdx.x | threadIdx.x) return;
    Fr z = Fr::zero();
    zero[0] = z;
#pragma nounroll
    for (uint32_t l = 0; l < depth; l++) { z = hash2(tab, f, p, z, z); zero[l + 1] = z; }
}

// one lane per old slot, out of place; the new table is empty and at least as large
__global__ __launch_bounds__(POS_THREADS) void smt_rehash_kernel(const uint64_t *__restrict__ old_keys, const Fr *__restrict__ old_vals, uint64_t old_cap,
                                                                  uint64_t *__restrict__ keys, Fr *__restrict__ vals, uint32_t log_cap, unsigned long long *err) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= old_cap) return;
    const uint64_t key = old_keys[s];
    if (key == SMT_EMPTY) return;
    const uint64_t to = smt_claim(keys, log_cap, key, nullptr, err);
    if (to != SMT_NOT_FOUND) vals[to] = old_vals[s];
}

// a level as merkle_plan.hpp's drivers see it
struct SmtStore {
    uint64_t *keys; Fr *vals; uint32_t log_cap; const Fr *zero_l; unsigned long long *count, *err;
    __device__ __forceinline__ void put(uint64_t key, const Fr &v) const {
        const uint64_t s = smt_claim(keys, log_cap, key, count, err);
        if (s != SMT_NOT_FOUND) vals[s] = v;
    }
    __device__ __forceinline__ const Fr *get(uint64_t key) const {
        const uint64_t s = smt_find(keys, log_cap, key, err);
        return s != SMT_NOT_FOUND ? vals + s : zero_l;
    }
};

// read only.  One lane per (proof, level): lane i * depth + l stores the sibling of indices[i] at level l
__global__ __launch_bounds__(POS_THREADS) void smt_siblings_kernel(SmtTables tabs, const Fr *__restrict__ zero, uint32_t depth, const uint64_t *__restrict__ idx, uint64_t total,
                                                                    Fr *__restrict__ sib, unsigned long long *err) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const uint64_t i = g / depth;
    const uint32_t l = (uint32_t)(g - i * depth);
    const SmtTable t = tabs.t[l];
    const uint64_t s = smt_find(t.keys, t.log_cap, (idx[i] >> l) ^ 1, err);
    sib[g] = s != SMT_NOT_FOUND ? t.vals[s] : zero[l];
}

// read only.  leaves[i] = the stored leaf at indices[i], or 0 (depth >= 1)
__global__ __launch_bounds__(POS_THREADS) void smt_leaves_kernel(const uint64_t *__restrict__ tkeys, const Fr *__restrict__ tvals, uint32_t log_cap,
                                                                  const uint64_t *__restrict__ idx, uint64_t n, Fr *__restrict__ leaves, unsigned long long *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = smt_find(tkeys, log_cap, idx[i], err);
    leaves[i] = s != SMT_NOT_FOUND ? tvals[s] : Fr::zero();
}

__global__ __launch_bounds__(POS_THREADS) void smt_fill_kernel(Fr *__restrict__ out, uint64_t n, const Fr *__restrict__ value) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = *value;
}

// ------------------------------------------------------------------------------------------ host
static inline uint64_t smt_level_nodes(uint32_t depth, uint32_t l) { return (uint64_t)1 << (depth - l); }      // depth - l <= 63: no shift of 64
// the smallest table that holds `entries` at a load of one half
static inline uint32_t smt_log_cap_for(uint64_t entries) {
    uint32_t lg = SMT_MIN_LOG;
    while (lg < 63 && ((uint64_t)1 << (lg - 1)) < entries) lg++;
    return lg;
}
static inline size_t smt_slot_bytes() { return sizeof(uint64_t) + sizeof(Fr); }

static int smt_args(fk_ctx *ctx, const fk_smt *t) {
    if (!t) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (t->ctx != ctx) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: the tree belongs to another context");
    return FK_OK;
}

// the counts and the error word of the download queued last, if it has arrived (wait: wait for it)
static int smt_take_counts(fk_ctx *ctx, fk_smt *t, bool wait) {
    if (t->pending) {
        if (wait) FK_HIP(ctx, hipEventSynchronize(t->ev));
        else {
            const hipError_t e = hipEventQuery(t->ev);
            if (e == hipErrorNotReady) { (void)hipGetLastError(); return FK_OK; }
            FK_HIP(ctx, e);
        }
        t->pending = false;
        for (uint32_t l = 0; l < t->depth; l++) t->lv[l].count = t->lv[l].bound = t->h_meta[l];
        if (t->h_meta[SMT_META_ERR]) t->broken = true;
    }
    return FK_OK;
}

static int smt_usable(fk_ctx *ctx, const fk_smt *t) {
    if (t->broken) FK_SET_ERR(ctx, FK_ERR_HIP, "sparse merkle: a probe of an earlier call ran through a whole table (error word %llu): the tree is not to be trusted",
                              (unsigned long long)t->h_meta[SMT_META_ERR]);
    return FK_OK;
}

static int smt_queue_counts(fk_ctx *ctx, fk_smt *t) {
    FK_HIP(ctx, hipMemcpyAsync(t->h_meta, t->d_meta, SMT_META_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipEventRecord(t->ev, ctx->stream));
    t->pending = true;
    return FK_OK;
}

struct SmtNewTable { uint64_t *keys = nullptr; Fr *vals = nullptr; uint32_t log_cap = 0; };
struct SmtGrowth {          // the tables a call allocates: freed here unless the tree took them
    SmtNewTable nt[FK_SMT_MAX_DEPTH];
    ~SmtGrowth() { for (auto &n : nt) { if (n.keys) (void)hipFree(n.keys); if (n.vals) (void)hipFree(n.vals); } }
};

static int smt_alloc_table(fk_ctx *ctx, uint32_t log_cap, SmtNewTable *n) {
    const uint64_t cap = (uint64_t)1 << log_cap;
    FK_HIP(ctx, hipMalloc((void **)&n->keys, cap * sizeof(uint64_t)));
    FK_HIP(ctx, hipMalloc((void **)&n->vals, cap * sizeof(Fr)));
    n->log_cap = log_cap;
    FK_HIP(ctx, hipMemsetAsync(n->keys, 0xff, cap * sizeof(uint64_t), ctx->stream));
    return FK_OK;
}

// room for k more writes on every level, before anything is written
static int smt_settle_capacity(fk_ctx *ctx, fk_smt *t, uint32_t k) {
    auto short_of_room = [&]() {
        for (uint32_t l = 0; l < t->depth; l++) {
            const fk_smt::Level &v = t->lv[l];
            if (v.bound + std::min<uint64_t>(k, smt_level_nodes(t->depth, l)) > ((uint64_t)1 << (v.log_cap - 1))) return true;
        }
        return false;
    };
    if (!short_of_room()) return FK_OK;
    FK_TRY(smt_take_counts(ctx, t, true));      // the bounds may be slack: the exact counts first
    FK_TRY(smt_usable(ctx, t));
    if (!short_of_room()) return FK_OK;
    SmtGrowth g;
    for (uint32_t l = 0; l < t->depth; l++) {
        const fk_smt::Level &v = t->lv[l];
        const uint64_t need = v.bound + std::min<uint64_t>(k, smt_level_nodes(t->depth, l));
        if (need > ((uint64_t)1 << (v.log_cap - 1))) FK_TRY(smt_alloc_table(ctx, smt_log_cap_for(need), &g.nt[l]));
    }
    // every allocation has succeeded: rehash, then the tree takes the new tables
    for (uint32_t l = 0; l < t->depth; l++) {
        SmtNewTable &n = g.nt[l];
        if (!n.keys) continue;
        fk_smt::Level &v = t->lv[l];
        const uint64_t old_cap = (uint64_t)1 << v.log_cap;
        hipLaunchKernelGGL(smt_rehash_kernel, dim3(pos_blocks(old_cap)), dim3(POS_THREADS), 0, ctx->stream, (const uint64_t *)v.keys, (const Fr *)v.vals, old_cap, n.keys, n.vals,
                           n.log_cap, t->d_meta + SMT_META_ERR);
        FK_HIP(ctx, hipGetLastError());
        std::swap(v.keys, n.keys); std::swap(v.vals, n.vals); v.log_cap = n.log_cap;      // (the old ones go with `g`: hipFree waits for the rehash)
    }
    FK_DBG(ctx, "sparse merkle: growth");
    return FK_OK;
}

static size_t smt_device_bytes(const fk_smt *t) {
    size_t b = t->block_bytes;
    for (uint32_t l = 0; l < t->depth; l++) b += smt_slot_bytes() << t->lv[l].log_cap;
    return b;
}

static SmtStore smt_store(const fk_smt *t, uint32_t l) {
    const fk_smt::Level &v = t->lv[l];
    return SmtStore{v.keys, v.vals, v.log_cap, t->d_zero + l, t->d_meta + l, t->d_meta + SMT_META_ERR};
}

// what the update and the set share in front of their levels: the tree usable, the indices good
static int smt_write_head(fk_ctx *ctx, fk_smt *t, const uint64_t *d_idx, uint32_t k, const char *what, const char *tail) {
    FK_TRY(smt_take_counts(ctx, t, false));
    FK_TRY(smt_usable(ctx, t));
    // the indices first: nothing is written, and no table grows, before they are known to be good
    PosDev d; FK_TRY(misc_head(ctx, nullptr, nullptr, 0, &d));
    return ms_check_indices(ctx, d.flag, d_idx, k, t->depth, "sparse merkle", what, tail);
}

// room for the k writes, before anything is written; from here on the tables may hold up to this much more
static int smt_make_room(fk_ctx *ctx, fk_smt *t, uint32_t k) {
    FK_TRY(smt_settle_capacity(ctx, t, k));
    for (uint32_t l = 0; l < t->depth; l++) t->lv[l].bound += ms_level_bound(t->depth, l, k);
    return FK_OK;
}

// k >= 1, arguments checked, the staging claimed.  ms: null, or where the timed entry wants the device times (then the call waits for the stream)
static int smt_update_dev(fk_ctx *ctx, fk_smt *t, const uint64_t *d_idx, const Fr *d_new, uint32_t k, Fr *d_old, Fr *d_sib, Fr *d_roots, double *ms) {
    const uint32_t depth = t->depth;
    FK_TRY(smt_write_head(ctx, t, d_idx, k, "update", MU_UPDATE_TAIL));
    if (depth == 0) return mu_update_depth0(ctx, d_new, k, t->d_root, d_old, d_roots, ms);
    MuScratch s; FK_TRY(mu_reserve(ctx, d_idx, depth, k, &s));
    MuEvents tm;
    if (ms) FK_HIP(ctx, tm.make(2 + 2 * (size_t)depth));
    FK_TRY(smt_make_room(ctx, t, k));
    auto store_at = [&](uint32_t l) { return smt_store(t, l); };
    FK_TRY(mu_update_levels(ctx, (const Fr *)t->d_tab, t->h.f, t->h.p, depth, d_idx, d_new, k, s, store_at, t->d_root, d_old, d_sib, d_roots, ms ? &tm : nullptr));
    FK_TRY(smt_queue_counts(ctx, t));
    return ms ? mu_finish_timed(ctx, tm, depth, ms) : FK_OK;
}

static int smt_update_args(fk_ctx *ctx, const fk_smt *t, size_t k) {
    FK_TRY(smt_args(ctx, t));
    if (k > FK_SMT_MAX_WRITES) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: one update takes at most 2^28 writes (got %zu)", k);
    return FK_OK;
}

// k >= 1, arguments checked, the staging claimed.  timed: null, or what the timed entry wants (then the call waits for the stream)
static int smt_set_dev(fk_ctx *ctx, fk_smt *t, const uint64_t *d_idx, const Fr *d_leaves, uint32_t k, Fr *d_root, const MsTimed *timed) {
    const uint32_t depth = t->depth;
    FK_TRY(smt_write_head(ctx, t, d_idx, k, "set", MS_SET_TAIL));
    if (depth == 0) return ms_set_depth0(ctx, d_leaves, k, t->d_root, d_root, timed);
    MsScratch s; FK_TRY(ms_reserve(ctx, d_idx, depth, k, &s));
    MuEvents tm;
    if (timed) FK_HIP(ctx, tm.make(2 + 2 * (size_t)depth));
    FK_TRY(smt_make_room(ctx, t, k));
    auto store_at = [&](uint32_t l) { return smt_store(t, l); };
    FK_TRY(ms_set_levels(ctx, (const Fr *)t->d_tab, t->h.f, t->h.p, depth, d_idx, d_leaves, k, s, store_at, t->d_root, d_root, timed ? &tm : nullptr));
    FK_TRY(smt_queue_counts(ctx, t));
    if (timed) FK_TRY(ms_finish_timed(ctx, tm, depth, s, *timed));
    return FK_OK;
}

// the end of a host-array entry that wrote: the counts have arrived with the outputs
static int smt_host_end(fk_ctx *ctx, fk_smt *t, int rc) {
    if (rc == FK_OK) rc = smt_take_counts(ctx, t, false);
    return rc == FK_OK ? smt_usable(ctx, t) : rc;
}

// n >= 1, arguments checked.  Read only: the tables, `misc` for the flag
static int smt_proofs_dev(fk_ctx *ctx, const fk_smt *t, const uint64_t *d_idx, size_t n, Fr *d_leaves, Fr *d_sib) {
    const uint32_t depth = t->depth;
    PosDev d; FK_TRY(misc_head(ctx, nullptr, nullptr, 0, &d));
    FK_TRY(ms_check_indices(ctx, d.flag, d_idx, (uint32_t)n, depth, "sparse merkle", "proofs", ""));
    unsigned long long *err = t->d_meta + SMT_META_ERR;
    if (d_leaves) {
        if (depth == 0) hipLaunchKernelGGL(smt_fill_kernel, dim3(pos_blocks(n)), dim3(POS_THREADS), 0, ctx->stream, d_leaves, (uint64_t)n, (const Fr *)t->d_root);
        else hipLaunchKernelGGL(smt_leaves_kernel, dim3(pos_blocks(n)), dim3(POS_THREADS), 0, ctx->stream, (const uint64_t *)t->lv[0].keys, (const Fr *)t->lv[0].vals,
                                t->lv[0].log_cap, d_idx, (uint64_t)n, d_leaves, err);
        FK_HIP(ctx, hipGetLastError());
    }
    if (d_sib && depth) {
        SmtTables tabs;
        for (uint32_t l = 0; l < depth; l++) tabs.t[l] = SmtTable{t->lv[l].keys, t->lv[l].vals, t->lv[l].log_cap};
        for (uint32_t l = depth; l < FK_SMT_MAX_DEPTH; l++) tabs.t[l] = SmtTable{nullptr, nullptr, 0};
        const uint64_t total = (uint64_t)n * depth;
        hipLaunchKernelGGL(smt_siblings_kernel, dim3(pos_blocks(total)), dim3(POS_THREADS), 0, ctx->stream, tabs, (const Fr *)t->d_zero, depth, d_idx, total, d_sib, err);
        FK_HIP(ctx, hipGetLastError());
    }
    return FK_OK;
}

static void smt_destroy(fk_smt *t) {
    for (auto &v : t->lv) { if (v.keys) (void)hipFree(v.keys); if (v.vals) (void)hipFree(v.vals); }
    if (t->d_block) (void)hipFree(t->d_block);
    if (t->h_meta) (void)hipHostFree(t->h_meta);
    if (t->ev) (void)hipEventDestroy(t->ev);
    delete t;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_smt_new(fk_ctx *ctx, const fk_poseidon *h, uint32_t depth, uint64_t expected_leaves, fk_smt **out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!h || !out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (h->t != 3) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: the tree hashes pairs with t = 3 parameters (got t = %u)", h->t);
    if (depth > FK_SMT_MAX_DEPTH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: depth %u is above the maximum of %u (a node index keeps one value for the empty slot)", depth, FK_SMT_MAX_DEPTH);
    FK_HIP(ctx, hipSetDevice(ctx->device));
    fk_smt *t = new fk_smt;
    struct Guard { fk_smt *t; ~Guard() { if (t) smt_destroy(t); } } guard{t};
    t->ctx = ctx; t->depth = depth; t->h = *h;
    t->zero.resize(depth + 1);
    const size_t tab_bytes = h->tab.size() * sizeof(Fr), zero_bytes = (size_t)(depth + 1) * sizeof(Fr);
    t->block_bytes = tab_bytes + zero_bytes + sizeof(Fr) + SMT_META_WORDS * sizeof(uint64_t);
    FK_HIP(ctx, hipMalloc(&t->d_block, t->block_bytes));
    t->d_tab = (Fr *)t->d_block; t->d_zero = t->d_tab + h->tab.size(); t->d_root = t->d_zero + depth + 1;
    t->d_meta = (unsigned long long *)(t->d_root + 1);
    FK_HIP(ctx, hipHostMalloc((void **)&t->h_meta, SMT_META_WORDS * sizeof(uint64_t)));
    memset(t->h_meta, 0, SMT_META_WORDS * sizeof(uint64_t));
    FK_HIP(ctx, hipEventCreateWithFlags(&t->ev, hipEventDisableTiming));
    for (uint32_t l = 0; l < depth; l++) {
        SmtNewTable n;
        const int rc = smt_alloc_table(ctx, smt_log_cap_for(std::min(expected_leaves, smt_level_nodes(depth, l))), &n);
        t->lv[l].keys = n.keys; t->lv[l].vals = n.vals; t->lv[l].log_cap = n.log_cap;      // the tree owns them, a failed pair included
        FK_TRY(rc);
    }
    FK_HIP(ctx, hipMemcpyAsync(t->d_tab, h->tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    FK_HIP(ctx, hipMemsetAsync(t->d_meta, 0, SMT_META_WORDS * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(smt_defaults_kernel, dim3(1), dim3(64), 0, ctx->stream, (const Fr *)t->d_tab, h->f, h->p, depth, t->d_zero);
    FK_HIP(ctx, hipGetLastError());
    FK_HIP(ctx, hipMemcpyAsync(t->d_root, t->d_zero + depth, sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(t->zero.data(), t->d_zero, zero_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    guard.t = nullptr;
    *out = t;
    return FK_OK;
}); }

void fk_smt_free(fk_ctx *ctx, fk_smt *t) {
    if (!t) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    smt_destroy(t);
}

int fk_smt_info(fk_ctx *ctx, const fk_smt *tc, uint64_t out[4]) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_args(ctx, tc));
    if (!out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    fk_smt *t = const_cast<fk_smt *>(tc);       // (the host's copy of the counts is a cache)
    FK_HIP(ctx, hipSetDevice(ctx->device));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FK_TRY(smt_take_counts(ctx, t, true));
    FK_TRY(smt_usable(ctx, t));
    uint64_t nodes = 0;
    for (uint32_t l = 0; l < t->depth; l++) nodes += t->lv[l].count;
    out[0] = t->depth; out[1] = t->depth ? t->lv[0].count : 1; out[2] = nodes; out[3] = smt_device_bytes(t);
    return FK_OK;
}); }

int fk_smt_defaults(const fk_smt *t, uint64_t *out) {
    if (!t || !out) return FK_ERR_BAD_ARG;
    for (uint32_t l = 0; l <= t->depth; l++) fr_to_limbs(t->zero[l], out + 4 * l);
    return FK_OK;
}

int fk_smt_root(fk_ctx *ctx, const fk_smt *t, uint64_t root[4]) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_args(ctx, t));
    if (!root) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));       // no scratch at all: runs beside an early front
    FK_HIP(ctx, hipMemcpyAsync(root, t->d_root, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

int fk_smt_update_timed_dev(fk_ctx *ctx, fk_smt *t, const void *d_indices, const void *d_new_leaves, size_t k, void *d_old_leaves, void *d_siblings, void *d_roots,
                            double ms[2]) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_update_args(ctx, t, k));
    if (ms) ms[0] = ms[1] = 0;
    if (!k) return FK_OK;
    if (!d_indices || !d_new_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "sparse merkle update"));      // smt_update_dev sorts in stage_a/b/c
    return smt_update_dev(ctx, t, (const uint64_t *)d_indices, (const Fr *)d_new_leaves, (uint32_t)k, (Fr *)d_old_leaves, (Fr *)d_siblings, (Fr *)d_roots, ms);
}); }

int fk_smt_update_dev(fk_ctx *ctx, fk_smt *t, const void *d_indices, const void *d_new_leaves, size_t k, void *d_old_leaves, void *d_siblings, void *d_roots) {
    return fk_smt_update_timed_dev(ctx, t, d_indices, d_new_leaves, k, d_old_leaves, d_siblings, d_roots, nullptr);
}

int fk_smt_update(fk_ctx *ctx, fk_smt *t, const uint64_t *indices, const uint64_t *new_leaves, size_t k, uint64_t *old_leaves, uint64_t *siblings, uint64_t *roots) {
    return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_update_args(ctx, t, k));
    if (!k) return FK_OK;
    if (!indices || !new_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "sparse merkle update"));
    MuArray a[] = {{new_leaves, nullptr, k}, {nullptr, old_leaves, k}, {nullptr, roots, k}, {nullptr, siblings, k * t->depth}};
    return smt_host_end(ctx, t, mu_host_call(ctx, indices, k, a, [&](const uint64_t *d_idx) {
        return smt_update_dev(ctx, t, d_idx, a[0].d, (uint32_t)k, a[1].d, a[3].d, a[2].d, nullptr);
    }));
}); }

int fk_smt_proofs_dev(fk_ctx *ctx, const fk_smt *t, const void *d_indices, size_t n, void *d_leaves, void *d_siblings) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_args(ctx, t));
    if (n > FK_SMT_MAX_WRITES) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: one call takes at most 2^28 proofs (got %zu)", n);
    if (!n) return FK_OK;
    if (!d_indices) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(smt_usable(ctx, t));
    FK_HIP(ctx, hipSetDevice(ctx->device));       // misc only: runs beside an early front
    return smt_proofs_dev(ctx, t, (const uint64_t *)d_indices, n, (Fr *)d_leaves, (Fr *)d_siblings);
}); }

int fk_smt_proofs(fk_ctx *ctx, const fk_smt *t, const uint64_t *indices, size_t n, uint64_t *leaves, uint64_t *siblings) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_args(ctx, t));
    if (n > FK_SMT_MAX_WRITES) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: one call takes at most 2^28 proofs (got %zu)", n);
    if (!n) return FK_OK;
    if (!indices) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(smt_usable(ctx, t));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    // a block of its own (no staging buffer: the call works during an early front)
    MuArray a[] = {{nullptr, leaves, n}, {nullptr, siblings, n * t->depth}};
    return mu_host_call(ctx, indices, n, a, [&](const uint64_t *d_idx) { return smt_proofs_dev(ctx, t, d_idx, n, a[0].d, a[1].d); });
}); }

int fk_smt_export_level(fk_ctx *ctx, const fk_smt *t, uint32_t level, uint64_t *keys, uint64_t *vals, size_t cap, size_t *n) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_args(ctx, t));
    if (!n || (keys && !vals)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (level > t->depth) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: level %u of a tree of depth %u", level, t->depth);
    FK_TRY(smt_usable(ctx, t));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    if (level == t->depth) {        // the root alone
        *n = 1;
        if (!keys) return FK_OK;
        if (cap < 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: level %u stores 1 entry, room for %zu", level, cap);
        keys[0] = 0;
        FK_HIP(ctx, hipMemcpyAsync(vals, t->d_root, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FK_OK;
    }
    // not a hot path: the whole table comes to the host and is ordered there
    const fk_smt::Level &v = t->lv[level];
    const size_t slots = (size_t)1 << v.log_cap;
    std::vector<uint64_t> hk(slots);
    FK_HIP(ctx, hipMemcpyAsync(hk.data(), v.keys, slots * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<std::pair<uint64_t, size_t>> have;      // (key, slot)
    for (size_t s = 0; s < slots; s++) if (hk[s] != SMT_EMPTY) have.emplace_back(hk[s], s);
    *n = have.size();
    if (!keys) return FK_OK;
    if (cap < have.size()) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "sparse merkle: level %u stores %zu entries, room for %zu", level, have.size(), cap);
    std::sort(have.begin(), have.end());
    std::vector<Fr> hv(slots);
    FK_HIP(ctx, hipMemcpyAsync(hv.data(), v.vals, slots * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < have.size(); i++) { keys[i] = have[i].first; fr_to_limbs(hv[have[i].second], vals + 4 * i); }
    return FK_OK;
}); }

// ---- include/fawkes_hip_merkle_set.h
int fk_smt_set_timed_dev(fk_ctx *ctx, fk_smt *t, const void *d_indices, const void *d_leaves, size_t k, void *d_root, double ms[2], uint64_t *distinct) {
    return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_update_args(ctx, t, k));
    if (ms) ms[0] = ms[1] = 0;
    if (!k) return FK_OK;
    if (!d_indices || !d_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "sparse merkle set"));      // merkle_plan.hpp's bulk write sorts and selects in stage_a/b/c
    const MsTimed timed{ms, distinct};
    return smt_set_dev(ctx, t, (const uint64_t *)d_indices, (const Fr *)d_leaves, (uint32_t)k, (Fr *)d_root, &timed);
}); }

int fk_smt_set_dev(fk_ctx *ctx, fk_smt *t, const void *d_indices, const void *d_leaves, size_t k, void *d_root) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_update_args(ctx, t, k));
    if (!k) return FK_OK;
    if (!d_indices || !d_leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "sparse merkle set"));
    return smt_set_dev(ctx, t, (const uint64_t *)d_indices, (const Fr *)d_leaves, (uint32_t)k, (Fr *)d_root, nullptr);
}); }

int fk_smt_set(fk_ctx *ctx, fk_smt *t, const uint64_t *indices, const uint64_t *leaves, size_t k, uint64_t root[4]) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(smt_update_args(ctx, t, k));
    if (!k) return FK_OK;
    if (!indices || !leaves) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "sparse merkle set"));
    MuArray a[] = {{leaves, nullptr, k}, {nullptr, root, 1}};
    return smt_host_end(ctx, t, mu_host_call(ctx, indices, k, a, [&](const uint64_t *d_idx) { return smt_set_dev(ctx, t, d_idx, a[0].d, (uint32_t)k, a[1].d, nullptr); }));
}); }

}  // extern "C"
