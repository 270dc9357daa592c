// Shared by merkle_update.hip (dense trees) and sparse_merkle.hip (sparse trees): the part of an ordered update that depends on the
// leaf indices alone -- the index check, the identity order the stable sort starts from, and the per-level plan (previous toucher of
// every write's sibling, and the next level's order, merkle_update.hip's header comment) -- with the small host helpers of both drivers.
// The kernels have internal linkage: each of the two translation units carries its own copy in its own code object.
#pragma once
#include "poseidon.hpp"

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

}  // namespace fk
