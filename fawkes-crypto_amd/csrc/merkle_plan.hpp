// Shared by merkle_update.hip (dense trees) and sparse_merkle.hip (sparse trees): everything about k leaf writes but how a level is
// stored.  A store is a small struct passed by value: put(key, value), and get(key) -> where the value of a stored node lies (the
// level's default where the store has none).  Both calls begin with the index check and ONE stable radix sort of the pairs (index, j)
// over the depth index bits; these sorts and the bulk write's select are the library's use of rocPRIM.
//
// The ordered update (include/fawkes_hip_merkle.h, fawkes_hip_sparse_merkle.h).  Write j of k replaces leaf idx[j]; it must see the
// tree as the writes 0 .. j - 1 left it.  At level l the only thing write j needs from elsewhere is the value of its SIBLING node at its
// own moment: the value left there by the latest earlier write i < j that passes through that node (its "previous toucher"), or the
// stored node when there is none.  Neither depends on level l of write j itself, so a level is ONE launch of k independent hashes, and
// no chain of dependent hashes is longer than the depth.  Who the previous toucher is depends on the indices alone: at level l the order
// array is sorted by (index >> l, j), so the writes through one node form a contiguous run, ascending in j.  Per level:
//   plan        one write per lane, by position q in the order: binary searches on the node keys give the run of the lane's own node
//               [a, b) and of the sibling node [c, d) (the two are neighbours: they share the parent), a binary search on j inside the
//               sibling run gives r = its writes earlier than j; the previous toucher is element r - 1 of that run; the lane's position
//               in the next level's order is min(a, c) + (q - a) + r -- the two runs merged by rank, no second sort
//   hash        one write per lane, by j: sib = the previous toucher's current value or what the store has; next[j] = H(cur[j], sib)
//               or H(sib, cur[j]); sib goes to siblings[j * depth + l].  The pointer is chosen first and loaded once, so whatever the
//               store's get needed is dead before the permutation: the register budget of the t = 3 hash kernels
//   write-back  the last write of each run puts its current value into the level's store -- in a launch of its own BEHIND the hash
//               launch of that level: a write j whose sibling has no earlier toucher reads the STORED node there, and a later write
//               i > j through that sibling would otherwise overwrite it first
// After the last level cur[j] is the root after write j.  The old leaf of a write is the new leaf of the previous element of its run at
// level 0, or what the store of level 0 has.  Scratch per call: cur / next (2 k Fr, ctx->stage_a); keys, next keys (k u64 each), order,
// next order, previous touchers (k u32 each) (ctx->stage_b); the sort's temporary storage (ctx->stage_c).
//
// The bulk write ("set", include/fawkes_hip_merkle_set.h).  The same check and the same stable sort; then the LAST element of every run
// of equal indices is selected into an ascending list of m_0 distinct (key, value) pairs, and per level l = 0 .. depth - 1:
//   write-back  one list element per lane: the level's store takes (key, value).  The keys are distinct
//   select      the heads of the runs of equal key >> 1 are the m_(l + 1) distinct parents: rocPRIM's select over the positions
//               0 .. bound - 1 writes the heads' positions, compacted, and their number -- to device memory, where the next launches
//               read it.  The host launches with its bound min(k, 2^(depth - l)); lanes at or past the device's count leave
//   hash        one PARENT per lane, lanes dense: lane i < m_(l + 1) takes head i.  Its other child is the head's neighbour in the
//               list, or is not in the list and is read from the level's store
// so a node is hashed once however many writes pass through it.  A node of level l is either in the list (written) or read as an
// absent child, never both, and the write-back is a launch of its own in FRONT of the hash launch of its level: the hash launch reads
// a store that no lane is writing, and nothing has to be argued about a probe beside a claim.
//
// The host-array entries of both files: one device block per call (mu_host_call).
//
// The kernels have internal linkage: each of the two translation units carries its own copy in its own code object.
#pragma once
#include "poseidon.hpp"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <algorithm>

namespace fk {

static constexpr uint32_t MU_NONE = 0xffffffffu;

static __global__ __launch_bounds__(POS_THREADS) void mu_check_kernel(const uint64_t *__restrict__ idx, uint32_t k, uint32_t depth, uint32_t *bad) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < k && (idx[j] >> depth)) atomicOr(bad, 1u);
}

static __global__ __launch_bounds__(POS_THREADS) void mu_iota_kernel(uint32_t *__restrict__ out, uint32_t k) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < k) out[j] = j;
}

// the first position in [lo, hi) whose element is not below x
template <class T>
static __device__ __forceinline__ uint32_t mu_lower_bound(const T *__restrict__ a, uint32_t lo, uint32_t hi, T x) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// keys[q] = index >> l of the write at position q, ord[q] = its j; sorted by (key, j)
static __global__ __launch_bounds__(POS_THREADS) void mu_plan_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ord, uint32_t k,
                                                                      uint32_t *__restrict__ prev, uint64_t *__restrict__ next_keys, uint32_t *__restrict__ next_ord) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t node = keys[q], left = node & ~(uint64_t)1;
    const uint32_t j = ord[q];
    // [lo, mid) = the writes through the left child of the parent, [mid, hi) = those through the right one; lo <= q < hi
    const uint32_t lo = mu_lower_bound(keys, 0u, q, left);
    const uint32_t mid = mu_lower_bound(keys, lo, k, left | 1);
    const uint32_t hi = mu_lower_bound(keys, mid > q ? mid : q, k, left + 2);
    const bool right = node & 1;
    const uint32_t a = right ? mid : lo, c = right ? lo : mid, d = right ? mid : hi;
    const uint32_t r = mu_lower_bound(ord, c, d, j) - c;
    prev[j] = r ? ord[c + r - 1] : MU_NONE;
    const uint32_t pos = lo + (q - a) + r;
    next_ord[pos] = j;
    next_keys[pos] = node >> 1;
}

struct MuEvents {       // HIP events of one timed call
    std::vector<hipEvent_t> ev;
    ~MuEvents() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    hipError_t make(size_t n) {
        for (size_t i = 0; i < n; i++) { hipEvent_t e; const hipError_t rc = hipEventCreate(&e); if (rc != hipSuccess) return rc; ev.push_back(e); }
        return hipSuccess;
    }
};

struct MuDevBlock {     // device copies of a host entry's arguments: freed on every path
    void *p = nullptr;
    ~MuDevBlock() { if (p) (void)hipFree(p); }
};

// one array of a host-array entry, n Fr long: uploaded from `in`, downloaded to `out`.  d: its device copy, null where the caller gave
// neither pointer (an output that was not asked for) or n is 0
struct MuArray { const uint64_t *in; uint64_t *out; size_t n; Fr *d; };

// One block: the arrays in their order | the k indices.  call(d_idx) runs between the uploads and the downloads; the block is in use
// until the stream has drained, on the error paths too
template <size_t N, class Call>
static int mu_host_call(fk_ctx *ctx, const uint64_t *indices, size_t k, MuArray (&arrays)[N], Call call) {
    size_t frs = 0;
    for (const MuArray &a : arrays) if (a.in || a.out) frs += a.n;
    MuDevBlock blk;
    FK_HIP(ctx, hipMalloc(&blk.p, frs * sizeof(Fr) + k * sizeof(uint64_t)));
    Fr *at = (Fr *)blk.p;
    for (MuArray &a : arrays) if ((a.in || a.out) && a.n) { a.d = at; at += a.n; }
    uint64_t *d_idx = (uint64_t *)at;
    auto run = [&]() -> int {
        FK_HIP(ctx, hipMemcpyAsync(d_idx, indices, k * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        for (const MuArray &a : arrays) if (a.d && a.in) FK_HIP(ctx, hipMemcpyAsync(a.d, a.in, a.n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        FK_TRY(call((const uint64_t *)d_idx));
        for (const MuArray &a : arrays) if (a.d && a.out) FK_HIP(ctx, hipMemcpyAsync(a.out, a.d, a.n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        return FK_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// the index check of every call: one flag comes to the host, and nothing has been written when it does.  what: "update", "set",
// "proofs"; tail: what the refusal left alone
static int ms_check_indices(fk_ctx *ctx, uint32_t *flag, const uint64_t *d_idx, uint32_t k, uint32_t depth, const char *tree, const char *what, const char *tail) {
    FK_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(mu_check_kernel, dim3(pos_blocks(k)), dim3(POS_THREADS), 0, ctx->stream, d_idx, k, depth, flag);
    FK_HIP(ctx, hipGetLastError());
    uint32_t bad = 0;
    FK_HIP(ctx, hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a leaf index of the %s is not below 2^%u (nothing was written%s)", tree, what, depth, tail);
    return FK_OK;
}
static constexpr const char *MU_UPDATE_TAIL = ": the tree and the outputs are as they were", *MS_SET_TAIL = ": the tree and the root output are as they were";

// the end of a timed call: the wait and the two times.  tm: [0], [1] around everything, [2 + 2 l], [3 + 2 l] around the hash launch of level l
static int mu_finish_timed(fk_ctx *ctx, const MuEvents &tm, uint32_t depth, double *ms) {
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ms) {
        float t = 0;
        FK_HIP(ctx, hipEventElapsedTime(&t, tm.ev[0], tm.ev[1]));
        ms[0] = t; ms[1] = 0;
        for (uint32_t l = 0; l < depth; l++) { FK_HIP(ctx, hipEventElapsedTime(&t, tm.ev[2 + 2 * l], tm.ev[3 + 2 * l])); ms[1] += t; }
    }
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ the ordered update
// level 0 only: what each write replaces.  keys / ord: the level-0 order; st0: the store of the leaves
template <class Store>
static __global__ __launch_bounds__(POS_THREADS) void mu_old_leaves_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ord, uint32_t k, Store st0,
                                                                            const Fr *__restrict__ new_leaves, Fr *__restrict__ old) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t node = keys[q];
    old[ord[q]] = (q > 0 && keys[q - 1] == node) ? new_leaves[ord[q - 1]] : *st0.get(node);
}

// st: the store of level l; cur: the writes' values at level l (by j); sib_out: siblings + l, or null
template <class Store>
static __global__ __launch_bounds__(POS_THREADS) void mu_hash_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, Store st, const uint64_t *__restrict__ idx, uint32_t l,
                                                                      uint32_t depth, const uint32_t *__restrict__ prev, const Fr *__restrict__ cur, uint32_t k,
                                                                      Fr *__restrict__ next, Fr *__restrict__ sib_out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint64_t node = idx[j] >> l;
    const uint32_t pj = prev[j];
    const Fr *from = pj != MU_NONE ? cur + pj : st.get(node ^ 1);
    const Fr sib = *from;
    const Fr own = cur[j];
    if (sib_out) sib_out[(size_t)j * depth] = sib;
    const bool right = node & 1;
    Fr x, y;
#pragma unroll
    for (int i = 0; i < 8; i++) { x.v[i] = right ? sib.v[i] : own.v[i]; y.v[i] = right ? own.v[i] : sib.v[i]; }
    next[j] = hash2(tab, f, p, x, y);
}

// the last write of each run leaves its value in the level's store.  Run-last lanes carry distinct keys
template <class Store>
static __global__ __launch_bounds__(POS_THREADS) void mu_write_back_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ord, uint32_t k,
                                                                            const Fr *__restrict__ cur, Store st) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t node = keys[q];
    if (q + 1 == k || keys[q + 1] != node) st.put(node, cur[ord[q]]);
}

// the staging of one call: cur / next | keys, next keys, order, next order, previous touchers | rocPRIM's temporary storage
struct MuScratch { Fr *val[2]; uint64_t *keys, *next_keys; uint32_t *ord, *next_ord, *prev; void *tmp; size_t sort_bytes; };

static int mu_reserve(fk_ctx *ctx, const uint64_t *d_idx, uint32_t depth, uint32_t k, MuScratch *s) {
    s->sort_bytes = 0;
    FK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, s->sort_bytes, d_idx, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)k, 0u, depth, ctx->stream));
    FK_HIP(ctx, ctx->stage_a.reserve((size_t)2 * k * sizeof(Fr)));
    FK_HIP(ctx, ctx->stage_b.reserve((size_t)k * (2 * sizeof(uint64_t) + 3 * sizeof(uint32_t))));
    FK_HIP(ctx, ctx->stage_c.reserve(s->sort_bytes ? s->sort_bytes : 8));
    s->val[0] = ctx->stage_a.as<Fr>(); s->val[1] = s->val[0] + k;
    s->keys = ctx->stage_b.as<uint64_t>(); s->next_keys = s->keys + k;
    s->ord = (uint32_t *)(s->next_keys + k); s->next_ord = s->ord + k; s->prev = s->next_ord + k;
    s->tmp = ctx->stage_c.p;
    return FK_OK;
}

// depth 0: the tree is its root, the one leaf, and every write replaces the one before it.  k >= 1; ms: null, or a timed call's times
static int mu_update_depth0(fk_ctx *ctx, const Fr *d_new, uint32_t k, Fr *root, Fr *d_old, Fr *d_roots, double *ms) {
    if (d_old) {
        FK_HIP(ctx, hipMemcpyAsync(d_old, root, sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
        if (k > 1) FK_HIP(ctx, hipMemcpyAsync(d_old + 1, d_new, (size_t)(k - 1) * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (d_roots) FK_HIP(ctx, hipMemcpyAsync(d_roots, d_new, (size_t)k * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(root, d_new + (k - 1), sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (ms) { FK_HIP(ctx, hipStreamSynchronize(ctx->stream)); ms[0] = ms[1] = 0; }
    return FK_OK;
}

// depth >= 1, k >= 1, the indices checked, `s` reserved (and, for a sparse tree, its capacity settled).  store_at(l): the store of
// level l.  Any of d_old, d_sib, d_roots may be null.  tm: null, or the events of a timed call (mu_finish_timed)
template <class StoreAt>
static int mu_update_levels(fk_ctx *ctx, const Fr *tab, uint32_t f, uint32_t p, uint32_t depth, const uint64_t *d_idx, const Fr *d_new, uint32_t k, const MuScratch &s,
                            StoreAt store_at, Fr *root, Fr *d_old, Fr *d_sib, Fr *d_roots, MuEvents *tm) {
    const dim3 grid(pos_blocks(k)), block(POS_THREADS);
    uint64_t *keys = s.keys, *next_keys = s.next_keys;
    uint32_t *ord = s.ord, *next_ord = s.next_ord;
    size_t bytes = s.sort_bytes;
    if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[0], ctx->stream));
    // the level-0 order: a stable sort of (index, j) by the index
    hipLaunchKernelGGL(mu_iota_kernel, grid, block, 0, ctx->stream, next_ord, k);
    FK_HIP(ctx, hipGetLastError());
    FK_HIP(ctx, rocprim::radix_sort_pairs(s.tmp, bytes, d_idx, keys, (const uint32_t *)next_ord, ord, (size_t)k, 0u, depth, ctx->stream));
    if (d_old) hipLaunchKernelGGL(mu_old_leaves_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys, (const uint32_t *)ord, k, store_at(0), d_new, d_old);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "merkle update: sort");
    const Fr *cur = d_new;
    for (uint32_t l = 0; l < depth; l++) {
        Fr *next = s.val[l & 1];
        const auto st = store_at(l);
        hipLaunchKernelGGL(mu_plan_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys, (const uint32_t *)ord, k, s.prev, next_keys, next_ord);
        if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[2 + 2 * l], ctx->stream));
        hipLaunchKernelGGL(mu_hash_kernel, grid, block, 0, ctx->stream, tab, f, p, st, d_idx, l, depth, (const uint32_t *)s.prev, cur, k, next, d_sib ? d_sib + l : (Fr *)nullptr);
        if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[3 + 2 * l], ctx->stream));
        hipLaunchKernelGGL(mu_write_back_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys, (const uint32_t *)ord, k, cur, st);
        FK_HIP(ctx, hipGetLastError());
        FK_DBG(ctx, "merkle update: level");
        std::swap(keys, next_keys); std::swap(ord, next_ord);
        cur = next;
    }
    // every write passes through the root: the last of the list leaves its value there
    if (d_roots) FK_HIP(ctx, hipMemcpyAsync(d_roots, cur, (size_t)k * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(root, cur + (k - 1), sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[1], ctx->stream));
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ the bulk write
// rocPRIM's select asks these of a position (a uint32_t from a counting iterator)
struct MsRunLast {          // keys: all k writes, sorted by (index, position)
    const uint64_t *keys; uint32_t k;
    __host__ __device__ bool operator()(uint32_t q) const { return q >= k - 1 || keys[q + 1] != keys[q]; }       // k >= 1
};
struct MsParentHead {       // keys: the *m distinct nodes of a level, ascending
    const uint64_t *keys; const size_t *m;
    __host__ __device__ bool operator()(uint32_t i) const { return i < *m && (i == 0 || (keys[i - 1] >> 1) != (keys[i] >> 1)); }
};

// level 0: src[i] = the position, in the sorted writes, of the last write to the i-th distinct index
static __global__ __launch_bounds__(POS_THREADS) void ms_gather_kernel(const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ ord, const Fr *__restrict__ leaves,
                                                                        const uint32_t *__restrict__ src, const size_t *__restrict__ m, uint32_t bound,
                                                                        uint64_t *__restrict__ keys, Fr *__restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bound || i >= *m) return;
    const uint32_t q = src[i];
    keys[i] = skeys[q];
    vals[i] = leaves[ord[q]];
}

template <class Store>
static __global__ __launch_bounds__(POS_THREADS) void ms_write_back_kernel(const uint64_t *__restrict__ keys, const Fr *__restrict__ vals, const size_t *__restrict__ m,
                                                                            uint32_t bound, Store st) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bound || i >= *m) return;
    st.put(keys[i], vals[i]);
}

// keys / vals: the m[0] nodes of the level; src: the positions of the m[1] heads; st: the level's store
template <class Store>
static __global__ __launch_bounds__(POS_THREADS) void ms_hash_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const uint64_t *__restrict__ keys,
                                                                      const Fr *__restrict__ vals, const uint32_t *__restrict__ src, const size_t *__restrict__ m,
                                                                      uint32_t bound, Store st, uint64_t *__restrict__ next_keys, Fr *__restrict__ next_vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bound || i >= m[1]) return;
    const uint32_t at = src[i];
    const uint64_t node = keys[at];
    // the head is the left child with the right one behind it, or the parent's only child in the list
    const bool pair = !(node & 1) && at + 1 < m[0] && keys[at + 1] == (node | 1);
    const Fr *from = pair ? vals + at + 1 : st.get(node ^ 1);
    const Fr sib = *from;
    const Fr own = vals[at];
    const bool right = node & 1;
    Fr x, y;
#pragma unroll
    for (int j = 0; j < 8; j++) { x.v[j] = right ? sib.v[j] : own.v[j]; y.v[j] = right ? own.v[j] : sib.v[j]; }
    next_keys[i] = node >> 1;
    next_vals[i] = hash2(tab, f, p, x, y);
}

static inline uint64_t ms_level_bound(uint32_t depth, uint32_t l, uint32_t k) { return std::min<uint64_t>(k, (uint64_t)1 << (depth - l)); }      // depth - l <= 63

struct MsTimed { double *ms; uint64_t *distinct; };     // what a timed entry wants back (either may be null): then the call waits for the stream

// the staging of one call, carved after every buffer has its size: list values | sorted keys, list keys, the counts m_0 .. m_depth,
// order, identity, positions | rocPRIM's temporary storage.  92 bytes per write and 8 * (depth + 1), the temporary storage apart
struct MsScratch {
    Fr *val[2]; uint64_t *key[2]; size_t *counts; uint32_t *ord, *iota, *src; void *tmp; size_t sort_bytes, select_bytes;
};

static int ms_reserve(fk_ctx *ctx, const uint64_t *d_idx, uint32_t depth, uint32_t k, MsScratch *s) {
    s->sort_bytes = s->select_bytes = 0;
    FK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, s->sort_bytes, d_idx, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)k, 0u, depth, ctx->stream));
    FK_HIP(ctx, rocprim::select(nullptr, s->select_bytes, rocprim::counting_iterator<uint32_t>(0), (uint32_t *)nullptr, (size_t *)nullptr, (size_t)k,
                                MsParentHead{nullptr, nullptr}, ctx->stream));
    size_t run_last = 0;
    FK_HIP(ctx, rocprim::select(nullptr, run_last, rocprim::counting_iterator<uint32_t>(0), (uint32_t *)nullptr, (size_t *)nullptr, (size_t)k, MsRunLast{nullptr, 0}, ctx->stream));
    s->select_bytes = std::max(s->select_bytes, run_last);
    FK_HIP(ctx, ctx->stage_a.reserve((size_t)2 * k * sizeof(Fr)));
    FK_HIP(ctx, ctx->stage_b.reserve((size_t)k * (2 * sizeof(uint64_t) + 3 * sizeof(uint32_t)) + (size_t)(depth + 1) * sizeof(size_t)));
    FK_HIP(ctx, ctx->stage_c.reserve(std::max<size_t>(std::max(s->sort_bytes, s->select_bytes), 8)));
    s->val[0] = ctx->stage_a.as<Fr>(); s->val[1] = s->val[0] + k;
    s->key[1] = ctx->stage_b.as<uint64_t>(); s->key[0] = s->key[1] + k;        // the sorted writes' keys lie where the list of level 1 goes
    s->counts = (size_t *)(s->key[0] + k);
    s->ord = (uint32_t *)(s->counts + depth + 1); s->iota = s->ord + k; s->src = s->iota + k;
    s->tmp = ctx->stage_c.p;
    return FK_OK;
}

// depth 0: the tree is its root, the one leaf, and the last write wins.  k >= 1
static int ms_set_depth0(fk_ctx *ctx, const Fr *d_leaves, uint32_t k, Fr *root, Fr *d_root_out, const MsTimed *timed) {
    FK_HIP(ctx, hipMemcpyAsync(root, d_leaves + (k - 1), sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (d_root_out) FK_HIP(ctx, hipMemcpyAsync(d_root_out, d_leaves + (k - 1), sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (timed) {
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (timed->ms) timed->ms[0] = timed->ms[1] = 0;
        if (timed->distinct) timed->distinct[0] = 1;
    }
    return FK_OK;
}

// depth >= 1, k >= 1, the indices checked, `s` reserved (and, for a sparse tree, its capacity settled).  store_at(l): the store of
// level l.  tm: null, or the events of a timed call: [0], [1] around everything, [2 + 2 l], [3 + 2 l] around the hash launch of level l
template <class StoreAt>
static int ms_set_levels(fk_ctx *ctx, const Fr *tab, uint32_t f, uint32_t p, uint32_t depth, const uint64_t *d_idx, const Fr *d_leaves, uint32_t k, const MsScratch &s,
                         StoreAt store_at, Fr *root, Fr *d_root_out, MuEvents *tm) {
    const dim3 block(POS_THREADS);
    const rocprim::counting_iterator<uint32_t> positions(0);
    size_t bytes = s.sort_bytes;
    if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[0], ctx->stream));
    hipLaunchKernelGGL(mu_iota_kernel, dim3(pos_blocks(k)), block, 0, ctx->stream, s.iota, k);
    FK_HIP(ctx, hipGetLastError());
    uint64_t *skeys = s.key[1];
    FK_HIP(ctx, rocprim::radix_sort_pairs(s.tmp, bytes, d_idx, skeys, (const uint32_t *)s.iota, s.ord, (size_t)k, 0u, depth, ctx->stream));
    bytes = s.select_bytes;
    FK_HIP(ctx, rocprim::select(s.tmp, bytes, positions, s.src, s.counts, (size_t)k, MsRunLast{skeys, k}, ctx->stream));
    hipLaunchKernelGGL(ms_gather_kernel, dim3(pos_blocks(k)), block, 0, ctx->stream, (const uint64_t *)skeys, (const uint32_t *)s.ord, d_leaves, (const uint32_t *)s.src,
                       (const size_t *)s.counts, k, s.key[0], s.val[0]);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "merkle set: sort");
    for (uint32_t l = 0; l < depth; l++) {
        const uint32_t here = (uint32_t)ms_level_bound(depth, l, k), above = (uint32_t)ms_level_bound(depth, l + 1, k);
        const uint64_t *keys = s.key[l & 1];
        const Fr *vals = s.val[l & 1];
        const size_t *m = s.counts + l;
        const auto st = store_at(l);
        hipLaunchKernelGGL(ms_write_back_kernel, dim3(pos_blocks(here)), block, 0, ctx->stream, keys, vals, m, here, st);
        FK_HIP(ctx, hipGetLastError());
        bytes = s.select_bytes;
        FK_HIP(ctx, rocprim::select(s.tmp, bytes, positions, s.src, s.counts + l + 1, (size_t)here, MsParentHead{keys, m}, ctx->stream));
        if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[2 + 2 * l], ctx->stream));
        hipLaunchKernelGGL(ms_hash_kernel, dim3(pos_blocks(above)), block, 0, ctx->stream, tab, f, p, keys, vals, (const uint32_t *)s.src, m, above, st, s.key[(l + 1) & 1],
                           s.val[(l + 1) & 1]);
        if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[3 + 2 * l], ctx->stream));
        FK_HIP(ctx, hipGetLastError());
        FK_DBG(ctx, "merkle set: level");
    }
    // the list of level `depth` is the root alone
    const Fr *top = s.val[depth & 1];
    FK_HIP(ctx, hipMemcpyAsync(root, top, sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (d_root_out) FK_HIP(ctx, hipMemcpyAsync(d_root_out, top, sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if (tm) FK_HIP(ctx, hipEventRecord(tm->ev[1], ctx->stream));
    return FK_OK;
}

// the end of a timed set: the wait, the two times, the counts
static int ms_finish_timed(fk_ctx *ctx, const MuEvents &tm, uint32_t depth, const MsScratch &s, const MsTimed &timed) {
    FK_TRY(mu_finish_timed(ctx, tm, depth, timed.ms));
    if (timed.distinct) {
        static_assert(sizeof(size_t) == sizeof(uint64_t), "the counts are downloaded as they lie");
        FK_HIP(ctx, hipMemcpy(timed.distinct, s.counts, (size_t)(depth + 1) * sizeof(size_t), hipMemcpyDeviceToHost));
    }
    return FK_OK;
}

}  // namespace fk
