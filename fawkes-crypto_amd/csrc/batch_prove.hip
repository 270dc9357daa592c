// Batch prover (include/fawkes_hip_batch.h): `count` proofs of ONE small circuit under ONE key, every stage with the proof index as
// a second grid dimension.  Per group of proofs the number of launches is fixed and the host blocks once, at the download of the proofs.
//
//   evaluation   one lane per (row, proof, matrix): CSR walk over the resident system, bellman's input rows included, zero behind the rows
//   quotient     the per-proof prover's: quotient_rows (ntt.hip) over the group's rows -- ntt_pass_kernel with blockIdx.y = proof, the
//                tables are the context's NttDomain
//   five sums    one set of kernels, templated on the coordinate field, over SHARED bases: bucket = (proof, window, |digit|) of the
//                signed digits of the canonical scalar.  histogram (vector atomics) -> one device scan over all buckets of the group
//                -> scatter of (base index, sign) by atomic cursor -> accumulation, one lane per SEGMENT of a bucket (a witness is
//                mostly bits: digit 1 of window 0 holds a third of the points) -> reduction, one wave per (proof, window) -> Horner
//                fold over the windows and normalisation, one lane per proof
//   assembly     the per-proof prover's: groth16_assemble (curve.hpp), one proof per lane; the Borsh bytes are written on the device
//
// The proof bytes depend on (key, witness, r, s) only -- every sum is normalised to affine before it is used -- so bucket order (the
// scatter is unordered), window width and grouping are free; tests/test_gpu_batch_prove.py compares with the per-proof prover byte by byte.
#include "common.hpp"
#include "ntt_domain.hpp"
#include "r1cs.hpp"
#include "batch_shared.hpp"
#include <rocprim/device/device_scan.hpp>
#include <chrono>
#include <string.h>

using namespace fk;

namespace fk {

static_assert(FK_BATCH_MAX_GROUP <= 65535, "the proof index is gridDim.y");

// ------------------------------------------------------------------------------------------ evaluation
struct BatchEvalArgs {
    const uint64_t *ptr[3];
    const uint32_t *col[3];
    const uint32_t *cidx[3];
    Fr *out[3];
};
// grid (ceil(m / 256), proofs, 3)
__global__ __launch_bounds__(256) void batch_eval_kernel(BatchEvalArgs a, const Fr *table, ZView zv, uint64_t num_gates, uint64_t rows, uint64_t m) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t p = blockIdx.y, mtx = blockIdx.z;
    if (t >= m) return;
    Fr acc = Fr::zero();
    if (t < num_gates) {
        const uint64_t *ptr = a.ptr[mtx]; const uint32_t *col = a.col[mtx]; const uint32_t *cidx = a.cidx[mtx];
        for (uint64_t k = ptr[t], e = ptr[t + 1]; k < e; k++) {
            Fr v = zv.z[zaddr(zv, p, col[k])];
            const uint32_t ci = cidx[k];
            if (ci) v = Fr::mul(v, table[ci]);
            acc = Fr::add(acc, v);
        }
    } else if (t < rows && mtx == 0) {
        acc = zv.z[zaddr(zv, p, (uint32_t)(t - num_gates))];       // bellman's extra rows: input_i * 0 = 0
    }
    a.out[mtx][(uint64_t)p * m + t] = acc;
}

static BatchEvalArgs bt_eval_args(const fk_r1cs_dev *r, Fr *a, Fr *b, Fr *c) {
    BatchEvalArgs ea;
    for (int k = 0; k < 3; k++) { ea.ptr[k] = r->ptr[k]; ea.col[k] = r->col[k]; ea.cidx[k] = r->cidx[k]; }
    ea.out[0] = a; ea.out[1] = b; ea.out[2] = c;
    return ea;
}

// zero behind the rows (fk_batch_quotient_dev: the caller's arrays); grid (ceil((m - n) / 256), proofs, 3)
__global__ __launch_bounds__(256) void batch_pad_kernel(Fr *a, Fr *b, Fr *c, uint64_t n, uint64_t m) {
    const uint64_t t = n + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    Fr *x = blockIdx.z == 0 ? a : (blockIdx.z == 1 ? b : c);
    x[(uint64_t)blockIdx.y * m + t] = Fr::zero();
}

// ------------------------------------------------------------------------------------------ multiplications over shared bases
struct ScalarSrc { ZView zv; const uint32_t *idx; uint32_t var_offset; };
static __device__ __forceinline__ Fr load_scalar(const ScalarSrc &s, uint32_t proof, uint32_t j) {
    return s.zv.z[zaddr(s.zv, proof, s.idx ? s.idx[j] : s.var_offset + j)];
}

// Signed digits of the canonical scalar, c bits per window, W = 254 / c + 1 windows (so W * c >= 255: the top window absorbs the last
// carry).  digit in [-2^(c-1) + 1, 2^(c-1)]; bucket (proof, window, |digit| - 1) of NB = 2^(c-1) per window.  A zero scalar and a zero digit
// enter no bucket.  SCATTER = false: the histogram; true: the entry (base index | sign << 31) goes to the bucket's next free place.
template <bool SCATTER>
__global__ __launch_bounds__(256) void batch_digits_kernel(ScalarSrc s, uint32_t n, uint32_t c, uint32_t W, uint32_t *counter, const uint32_t *off, uint32_t *entries) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (j >= n) return;
    const Fr k = Fr::from_mont(load_scalar(s, p, j));
    if (k.is_zero()) return;
    const uint32_t NB = 1u << (c - 1), mask = (1u << c) - 1;
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t o = w * c, word = o >> 5, sh = o & 31;
        uint32_t raw = word < 8 ? k.v[word] >> sh : 0;
        if (sh + c > 32 && word + 1 < 8) raw |= k.v[word + 1] << (32 - sh);
        raw = (raw & mask) + carry;
        const bool neg = raw > NB;
        const uint32_t dgt = neg ? (mask + 1) - raw : raw;
        carry = neg ? 1 : 0;
        if (!dgt) continue;
        const uint32_t b = (p * W + w) * NB + (dgt - 1);
        if (!SCATTER) atomicAdd(&counter[b], 1u);
        else entries[off[b] + atomicAdd(&counter[b], 1u)] = j | (neg ? 0x80000000u : 0u);
    }
}

// segments of each bucket; element nb (the scans' total) stays 0
__global__ __launch_bounds__(256) void batch_segcount_kernel(const uint32_t *hist, uint32_t nb, uint32_t seg, uint32_t *segcnt) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) segcnt[b] = (hist[b] + seg - 1) / seg;
}

// One lane per segment of at most `seg` entries of a bucket.  segoff (exclusive scan of the segment counts, nb + 1 elements) names the
// segments; lane k finds its bucket by bisection.  tmax: the launch's bound on the number of segments.
template <class F>
__global__ __launch_bounds__(256) void batch_accumulate_kernel(const Affine<F> *bases, const uint32_t *entries, const uint32_t *off, const uint32_t *segoff,
                                                               uint32_t nb, uint32_t seg, Xyzz<F> *partial, uint32_t tmax) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= tmax || k >= segoff[nb]) return;
    uint32_t lo = 0, hi = nb;                      // segoff[lo] <= k < segoff[hi]
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (segoff[mid] <= k) lo = mid; else hi = mid; }
    const uint32_t first = off[lo] + (k - segoff[lo]) * seg, bend = off[lo + 1];
    const uint32_t last = first + seg < bend ? first + seg : bend;
    Xyzz<F> acc = Xyzz<F>::inf();
    for (uint32_t e = first; e < last; e++) {
        const uint32_t v = entries[e];
        acc.add_mixed(affine_neg_if(bases[v & 0x7fffffffu], (v >> 31) != 0));
    }
    partial[k] = acc;
}

// One wave per (proof, window): grid (W, proofs), 64 lanes.  Lane l owns the S = max(1, NB / 64) buckets of digits l S + 1 .. (l + 1) S: walking them
// from the top with a running sum gives sum (d - l S) B_d; the slice's total times the small integer l S is added, and the 64 lane sums
// are folded through LDS.
template <class F>
__global__ __launch_bounds__(64) void batch_reduce_kernel(const Xyzz<F> *partial, const uint32_t *segoff, uint32_t c, uint32_t W, Xyzz<F> *wsum) {
    using X = Xyzz<F>;
    __shared__ uint4 raw[64 * sizeof(X) / sizeof(uint4)];
    X *sh = (X *)raw;
    const uint32_t lane = threadIdx.x, w = blockIdx.x, p = blockIdx.y;
    const uint32_t NB = 1u << (c - 1), S = NB >= 64 ? NB / 64 : 1, lanes = NB / S;
    const uint32_t base = (p * W + w) * NB;
    X run = X::inf(), acc = X::inf();
    if (lane < lanes) {
        for (uint32_t i = S; i-- > 0;) {
            const uint32_t b = base + lane * S + i;
            for (uint32_t t = segoff[b], e = segoff[b + 1]; t < e; t++) run.add(partial[t]);
            acc.add(run);
        }
        uint32_t mult = lane * S;
        if (mult && !run.is_inf()) {
            X t = X::inf();
            for (int bit = 31 - __clz(mult); bit >= 0; bit--) { t = X::dbl(t); if ((mult >> bit) & 1) t.add(run); }
            acc.add(t);
        }
    }
    sh[lane] = acc;
    __syncthreads();
    for (uint32_t o = 32; o; o >>= 1) {
        if (lane < o) { X a = sh[lane]; a.add(sh[lane + o]); sh[lane] = a; }
        __syncthreads();
    }
    if (lane == 0) wsum[p * W + w] = sh[0];
}

// Horner fold over the windows and normalisation: one lane per proof; the affine sum goes to out + proof * stride (raw layout, zeros = infinity)
template <class F>
__global__ __launch_bounds__(64) void batch_horner_kernel(const Xyzz<F> *wsum, uint32_t c, uint32_t W, uint32_t proofs, uint8_t *out, uint32_t stride) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= proofs) return;
    Xyzz<F> acc = wsum[p * W + W - 1];
    for (uint32_t w = W - 1; w-- > 0;) {
        for (uint32_t i = 0; i < c; i++) acc = Xyzz<F>::dbl(acc);
        acc.add(wsum[p * W + w]);
    }
    *(Affine<F> *)(out + (size_t)p * stride) = acc.to_affine();
}

// ------------------------------------------------------------------------------------------ assembly
// groth16_assemble (curve.hpp) for one part per proof: parts = proofs x FK_MSM_RESULT_BYTES (H, L, A, B1, B2 raw affine); the Borsh bytes are written here
__global__ __launch_bounds__(64) void batch_assemble_kernel(AssembleKey key, const uint8_t *parts, const Fr *r, const Fr *s, uint32_t proofs, uint8_t *out) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= proofs) return;
    const uint8_t *q = parts + (size_t)p * FK_MSM_RESULT_BYTES;
    const G1Xyzz H = G1Xyzz::from_affine(*(const G1Affine *)q), L = G1Xyzz::from_affine(*(const G1Affine *)(q + 64));
    const G1Xyzz A = G1Xyzz::from_affine(*(const G1Affine *)(q + 128)), B1 = G1Xyzz::from_affine(*(const G1Affine *)(q + 192));
    const G2Xyzz B2 = G2Xyzz::from_affine(*(const G2Affine *)(q + 256));
    groth16_assemble(key, H, L, A, B1, B2, r[p], s[p], (Fq *)(out + (size_t)p * FK_PROOF_BYTES));
}

// ------------------------------------------------------------------------------------------ plan (host)
static inline uint32_t bt_windows(uint32_t c) { return 254 / c + 1; }
// Window width for n points per proof: the cheapest by a count of field products -- n W mixed additions (10 products) in the accumulation,
// 2 W 2^(c-1) full additions (14) in the reduction's bucket walk, and per window the 64 lanes' small multiple and LDS fold.
static uint32_t bt_choose_bits(uint64_t n) {
    uint32_t best = 4; double best_cost = 0;
    for (uint32_t c = 4; c <= FK_BATCH_WINDOW_BITS_MAX; c++) {      // (below 4 bits the window count alone rules a width out; forced widths go down to FK_BATCH_WINDOW_BITS_MIN)
        const double W = bt_windows(c), NB = (double)(1u << (c - 1));
        const double cost = 10.0 * (double)n * W + 28.0 * W * NB + W * 64.0 * (9.0 * c + 14.0 * c / 2 + 6 * 14.0);
        if (best_cost == 0 || cost < best_cost) { best = c; best_cost = cost; }
    }
    return best;
}
static uint32_t bt_segment(uint64_t n) {      // about sqrt(n / 2): the largest bucket of a witness (a third of the points) then costs as many partial sums as a segment costs entries
    uint32_t s = 16;
    while (s < 256 && (uint64_t)s * s * 2 < n) s <<= 1;
    return s;
}
static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct BtMsmShape { uint32_t c, W, NB, seg; uint64_t nb, max_entries, tmax; };
static BtMsmShape bt_msm_shape(uint64_t n, uint32_t c, uint32_t seg, uint32_t proofs) {
    BtMsmShape s;
    s.c = c; s.W = bt_windows(c); s.NB = 1u << (c - 1); s.seg = seg;
    s.nb = (uint64_t)proofs * s.W * s.NB;
    s.max_entries = (uint64_t)proofs * n * s.W;
    s.tmax = s.max_entries / seg + s.nb;           // every non-empty bucket has at most one segment that is not full
    return s;
}
// device scratch of the multiplications of one group: the largest of them
static uint64_t bt_msm_scratch(uint64_t n, uint32_t c1, uint32_t c2, uint32_t seg, uint32_t proofs) {
    const BtMsmShape a = bt_msm_shape(n, c1, seg, proofs), b = bt_msm_shape(n, c2, seg, proofs);
    const uint64_t nb = std::max(a.nb, b.nb), ent = std::max(a.max_entries, b.max_entries);
    return up256(3 * (nb + 1) * 4) + up256(ent * 4) + std::max(up256(a.tmax * sizeof(G1Xyzz)), up256(b.tmax * sizeof(G2Xyzz)))
         + std::max(up256((uint64_t)proofs * a.W * sizeof(G1Xyzz)), up256((uint64_t)proofs * b.W * sizeof(G2Xyzz))) + (1u << 20) /* the scans' temporary */;
}
static bool bt_msm_indexable(uint64_t n, uint32_t c1, uint32_t c2, uint32_t seg, uint32_t proofs) {
    for (uint32_t c : {c1, c2}) { const BtMsmShape s = bt_msm_shape(n, c, seg, proofs); if (s.nb >= (1ull << 31) || s.max_entries >= (1ull << 31) || s.tmax >= (1ull << 31)) return false; }
    return true;
}
static uint64_t bt_group_scratch(uint64_t m, uint64_t nmax, uint32_t c1, uint32_t c2, uint32_t seg, uint32_t g) {
    return up256(6 * (uint64_t)g * m * sizeof(Fr)) + bt_msm_scratch(nmax, c1, c2, seg, g)
         + up256((uint64_t)g * (2 * sizeof(Fr) + FK_MSM_RESULT_BYTES + FK_PROOF_BYTES));
}

static constexpr uint32_t BT_LAUNCHES_FRONT = 7, BT_LAUNCHES_BACK = 3;      // memset, histogram, segment counts, two scans, memset, scatter | accumulate, reduce, Horner

static int bt_plan(std::string &err, uint64_t m, uint64_t n_l, uint64_t n_a, uint64_t n_b, uint32_t count, const fk_batch_opts *opts, fk_batch_plan_info *out) {
    char buf[256];
    auto fail = [&](const char *msg) { err = msg; return FK_ERR_BAD_ARG; };
    if (!out) return fail("batch plan: null argument");
    memset(out, 0, sizeof *out);
    if (m < 2 || (m & (m - 1))) return fail("batch plan: the domain is not a power of two >= 2");
    if (m > ((uint64_t)1 << FK_BATCH_MAX_LOG_M)) {
        snprintf(buf, sizeof buf, "batch plan: domain %llu > 2^%d: one proof fills the device, use fk_prove_r1cs_dev", (unsigned long long)m, FK_BATCH_MAX_LOG_M);
        return fail(buf);
    }
    if (n_l >= ((uint64_t)1 << 31) || n_a >= ((uint64_t)1 << 31) || n_b >= ((uint64_t)1 << 31)) return fail("batch plan: a query does not fit 31-bit base indices");
    uint32_t c1 = opts ? opts->window_bits_g1 : 0, c2 = opts ? opts->window_bits_g2 : 0;
    for (uint32_t c : {c1, c2})
        if (c && (c < FK_BATCH_WINDOW_BITS_MIN || c > FK_BATCH_WINDOW_BITS_MAX)) {
            snprintf(buf, sizeof buf, "batch plan: window bits %u outside %d..%d", c, FK_BATCH_WINDOW_BITS_MIN, FK_BATCH_WINDOW_BITS_MAX);
            return fail(buf);
        }
    const uint64_t nmax = std::max(std::max(m - 1, n_l), std::max(n_a, n_b));
    if (!c1) c1 = bt_choose_bits(nmax);
    if (!c2) c2 = c1;                          // equal widths: B2 reuses B1's buckets (same scalars)
    const uint32_t seg = bt_segment(nmax);
    const uint64_t budget = opts && opts->scratch_budget_bytes ? opts->scratch_budget_bytes : FK_BATCH_PLAN_DEFAULT_BUDGET;
    uint32_t cap = count ? count : 1;
    if (cap > FK_BATCH_MAX_GROUP) cap = FK_BATCH_MAX_GROUP;
    auto fits = [&](uint32_t g) { return bt_msm_indexable(nmax, c1, c2, seg, g) && (uint64_t)g * m < ((uint64_t)1 << 31) && bt_group_scratch(m, nmax, c1, c2, seg, g) <= budget; };
    uint32_t g = 1;
    if (fits(cap)) g = cap;
    else { uint32_t lo = 1, hi = cap; while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (fits(mid)) lo = mid; else hi = mid; } g = lo; }      // scratch grows with g: bisection
    if (g == 1 && !bt_msm_indexable(nmax, c1, c2, seg, 1)) return fail("batch plan: one proof's buckets do not fit 31-bit indices");
    const uint32_t passes = ceil_log2_u64(m) ? (ceil_log2_u64(m) + 8) / 9 : 1;
    out->group = g; out->n_groups = count ? (count + g - 1) / g : 0;
    out->window_bits_g1 = c1; out->windows_g1 = bt_windows(c1);
    out->window_bits_g2 = c2; out->windows_g2 = bt_windows(c2);
    out->segment = seg; out->ntt_passes = passes;
    out->scratch_bytes = bt_group_scratch(m, nmax, c1, c2, seg, g);
    // evaluation; six transforms (+ one copy when a transform is a single pass and cannot run in place); H, L, A, B1 whole, B2 whole or
    // (equal widths) behind B1's buckets; assembly
    out->launches_per_group = 1 + 6 * passes + (passes == 1 ? 1 : 0) + 4 * (BT_LAUNCHES_FRONT + BT_LAUNCHES_BACK) + (c1 == c2 ? BT_LAUNCHES_BACK : BT_LAUNCHES_FRONT + BT_LAUNCHES_BACK) + 1;
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ drivers (host)
// histogram | bucket offsets | segment offsets: three runs of nb + 1 counters of the shape at hand
struct BtMsmBufs {
    uint32_t *sort, *entries; void *partial, *wsum;
    uint32_t *hist(const BtMsmShape &) const { return sort; }
    uint32_t *off(const BtMsmShape &s) const { return sort + (s.nb + 1); }
    uint32_t *segoff(const BtMsmShape &s) const { return sort + 2 * (s.nb + 1); }
};
static int bt_msm_reserve(fk_ctx *ctx, uint64_t n, uint32_t c1, uint32_t c2, uint32_t seg, uint32_t proofs, BtMsmBufs *b) {
    const BtMsmShape s1 = bt_msm_shape(n, c1, seg, proofs), s2 = bt_msm_shape(n, c2, seg, proofs);
    const uint64_t nb = std::max(s1.nb, s2.nb);
    FK_HIP(ctx, ctx->bt_sort.reserve(3 * (nb + 1) * 4 + 64));
    FK_HIP(ctx, ctx->bt_entries.reserve(std::max(s1.max_entries, s2.max_entries) * 4 + 64));
    FK_HIP(ctx, ctx->bt_partial.reserve(std::max(s1.tmax * sizeof(G1Xyzz), s2.tmax * sizeof(G2Xyzz)) + 64));
    FK_HIP(ctx, ctx->bt_wsum.reserve(std::max((uint64_t)proofs * s1.W * sizeof(G1Xyzz), (uint64_t)proofs * s2.W * sizeof(G2Xyzz)) + 64));
    b->sort = ctx->bt_sort.as<uint32_t>();
    b->entries = ctx->bt_entries.as<uint32_t>(); b->partial = ctx->bt_partial.p; b->wsum = ctx->bt_wsum.p;
    return FK_OK;
}

// histogram, scans, scatter: leaves off / segoff / entries for bt_msm_back (BT_LAUNCHES_FRONT launches)
static int bt_msm_front(fk_ctx *ctx, const ScalarSrc &src, uint32_t n, const BtMsmShape &s, uint32_t proofs, const BtMsmBufs &b) {
    const size_t nb1 = (size_t)s.nb + 1;
    uint32_t *hist = b.hist(s), *off = b.off(s), *segoff = b.segoff(s);
    FK_HIP(ctx, hipMemsetAsync(hist, 0, 2 * nb1 * 4, ctx->stream));          // histogram and (in `off` until the scan that fills it) the segment counts
    uint32_t *segcnt = off;
    const dim3 grid((n + 255) / 256, proofs);
    hipLaunchKernelGGL(batch_digits_kernel<false>, grid, dim3(256), 0, ctx->stream, src, n, s.c, s.W, hist, (const uint32_t *)nullptr, (uint32_t *)nullptr);
    FK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(batch_segcount_kernel, dim3((unsigned)((s.nb + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t *)hist, (uint32_t)s.nb, s.seg, segcnt);
    FK_HIP(ctx, hipGetLastError());
    size_t tmp_bytes = 0;
    FK_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp_bytes, segcnt, segoff, 0u, nb1, rocprim::plus<uint32_t>(), ctx->stream));
    FK_HIP(ctx, ctx->bt_scan.reserve(tmp_bytes + 256));
    FK_HIP(ctx, rocprim::exclusive_scan(ctx->bt_scan.p, tmp_bytes, segcnt, segoff, 0u, nb1, rocprim::plus<uint32_t>(), ctx->stream));
    FK_HIP(ctx, rocprim::exclusive_scan(ctx->bt_scan.p, tmp_bytes, hist, off, 0u, nb1, rocprim::plus<uint32_t>(), ctx->stream));
    FK_HIP(ctx, hipMemsetAsync(hist, 0, nb1 * 4, ctx->stream));              // now the scatter's cursors
    hipLaunchKernelGGL(batch_digits_kernel<true>, grid, dim3(256), 0, ctx->stream, src, n, s.c, s.W, hist, (const uint32_t *)off, b.entries);
    FK_HIP(ctx, hipGetLastError());
    return FK_OK;
}

// accumulate, reduce, Horner (BT_LAUNCHES_BACK launches); out + proof * stride receives the affine sum
template <class F>
static int bt_msm_back(fk_ctx *ctx, const Affine<F> *bases, const BtMsmShape &s, uint32_t proofs, const BtMsmBufs &b, uint8_t *out, uint32_t stride) {
    using X = Xyzz<F>;
    std::vector<EventPair> &ev = sizeof(F) == sizeof(Fq) ? ctx->ev_acc : ctx->ev_acc2;      // fk_stats_get: the accumulation's time; units = the launch's bound on the additions
    FK_TRY(stats_begin(ctx, ev, s.max_entries));
    hipLaunchKernelGGL(batch_accumulate_kernel<F>, dim3((unsigned)((s.tmax + 255) / 256)), dim3(256), 0, ctx->stream, bases, (const uint32_t *)b.entries,
                       (const uint32_t *)b.off(s), (const uint32_t *)b.segoff(s), (uint32_t)s.nb, s.seg, (X *)b.partial, (uint32_t)s.tmax);
    FK_HIP(ctx, hipGetLastError());
    FK_TRY(stats_end(ctx, ev));
    hipLaunchKernelGGL(batch_reduce_kernel<F>, dim3(s.W, proofs), dim3(64), 0, ctx->stream, (const X *)b.partial, (const uint32_t *)b.segoff(s), s.c, s.W, (X *)b.wsum);
    FK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(batch_horner_kernel<F>, dim3((proofs + 63) / 64), dim3(64), 0, ctx->stream, (const X *)b.wsum, s.c, s.W, proofs, out, stride);
    FK_HIP(ctx, hipGetLastError());
    return FK_OK;
}

// the budget an entry works with: the caller's, else a quarter of what is free now plus what the batch scratch already holds
static int bt_budget(fk_ctx *ctx, const fk_batch_opts *opts, fk_batch_opts *eff) {
    *eff = opts ? *opts : fk_batch_opts{0, 0, 0};
    if (eff->scratch_budget_bytes) return FK_OK;
    size_t free_b = 0, total_b = 0;
    FK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    size_t held = 0;
    for (const DevBuf *b : {&ctx->bt_vec, &ctx->bt_sort, &ctx->bt_entries, &ctx->bt_partial, &ctx->bt_wsum, &ctx->bt_io, &ctx->bt_scan, &ctx->bt_check}) held += b->cap;
    eff->scratch_budget_bytes = (free_b + held) / FK_BATCH_BUDGET_FREE_DIVISOR;
    if (!eff->scratch_budget_bytes) eff->scratch_budget_bytes = 1;
    return FK_OK;
}

// the claim of every batch entry: the device, and nothing of a per-proof call outstanding
static int bt_claim(fk_ctx *ctx, const char *who) {
    FK_TRY(scratch_claim(ctx, who));
    for (const auto &w : ctx->wslot) if (w.pending) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a submitted proof is outstanding (call fk_prove_r1cs_wait first)", who);
    if (proof_holds_lanes(ctx)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: witness multiplications are in flight", who);
    for (const auto &t : ctx->tails) if (t.active) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a multiplication begun with a *_begin_* call has not been collected", who);
    return FK_OK;
}

static int bt_check_layout(fk_ctx *ctx, int z_layout, const char *who) {
    if (z_layout != FK_BATCH_Z_ROWS && z_layout != FK_BATCH_Z_TILED) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: unknown witness layout %d", who, z_layout);
    return FK_OK;
}

struct BtEvents {
    hipEvent_t ev[10] = {nullptr};
    bool on = false;
    int init(fk_ctx *ctx) { for (auto &e : ev) FK_HIP(ctx, hipEventCreate(&e)); on = true; return FK_OK; }
    int mark(fk_ctx *ctx, int i) { if (on) FK_HIP(ctx, hipEventRecord(ev[i], ctx->stream)); return FK_OK; }
    ~BtEvents() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};

// sink, check_ms: null for the unchecked entries.  With a sink the per-proof check (batch_check.hip) is queued between the evaluation and
// the quotient of each group, and the group's reports come down with the group's proofs.
static int prove_batch_dev_impl(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_z, int z_layout, uint32_t count,
                                const uint64_t *rr, const uint64_t *ss, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm,
                                const BatchCheckSink *sink = nullptr, double *check_ms = nullptr) {
    const char *who = sink ? "fk_prove_batch_checked_dev" : "fk_prove_batch_dev";
    if (tm) memset(tm, 0, sizeof *tm);
    if (check_ms) *check_ms = 0;
    if (count == 0) return FK_OK;
    if (!key || !r || !d_z || !rr || !ss || !out_proofs) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    if (sink && !sink->reports) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null reports", who);
    FK_TRY(bt_check_layout(ctx, z_layout, who));
    if (r->copies > 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a tiled system makes ONE proof of its %u copies; load one instance (fk_r1cs_load)", who, r->copies);
    if (key->shard_count != 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a sharded key (%u of %u)", who, key->shard_index, key->shard_count);
    if (key->m > ((uint64_t)1 << FK_BATCH_MAX_LOG_M))
        FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: domain %llu > 2^%d: one proof fills the device, use fk_prove_r1cs_dev", who, (unsigned long long)key->m, FK_BATCH_MAX_LOG_M);
    uint64_t rows = 0;
    FK_TRY(r1cs_fits_key(ctx, r, key, &rows));
    FK_TRY(queries_fit_key(ctx, &r->qidx, key));
    FK_TRY(key_arrays_whole(ctx, key));
    FK_TRY(key_delta_ok(ctx, key));
    FK_TRY(bt_claim(ctx, who));
    const auto t_begin = std::chrono::steady_clock::now();
    fk_batch_opts eff;
    FK_TRY(bt_budget(ctx, opts, &eff));
    fk_batch_plan_info plan;
    FK_TRY(bt_plan(ctx->err, key->m, key->n_l, key->n_a, key->n_b, count, &eff, &plan));
    const uint64_t m = key->m;
    const uint32_t log_m = ceil_log2_u64(m), G = plan.group, nvars = key->num_input + key->num_aux;
    const uint64_t nmax = std::max(std::max(m - 1, key->n_l), std::max(key->n_a, key->n_b));
    NttDomain *dom = nullptr;
    FK_TRY(get_domain(ctx, log_m, &dom));
    BtEvents evs;
    if (tm || check_ms) FK_TRY(evs.init(ctx));
    // scratch of one group
    FK_HIP(ctx, ctx->bt_vec.reserve(6 * (size_t)G * m * sizeof(Fr)));
    Fr *va = ctx->bt_vec.as<Fr>(), *vb = va + (size_t)G * m, *vc = vb + (size_t)G * m, *vh = vc + (size_t)G * m, *s1 = vh + (size_t)G * m, *s2 = s1 + (size_t)G * m;
    BtMsmBufs mb;
    FK_TRY(bt_msm_reserve(ctx, nmax, plan.window_bits_g1, plan.window_bits_g2, plan.segment, G, &mb));
    const size_t io_r = 0, io_s = up256((size_t)G * sizeof(Fr)), io_parts = 2 * io_s, io_out = io_parts + up256((size_t)G * FK_MSM_RESULT_BYTES);
    FK_HIP(ctx, ctx->bt_io.reserve(io_out + (size_t)G * FK_PROOF_BYTES));
    uint8_t *io = ctx->bt_io.as<uint8_t>();
    if (sink) FK_TRY(batch_check_reserve(ctx, G));
    const AssembleKey ak = key->assemble_key();
    const BatchEvalArgs ea = bt_eval_args(r, va, vb, vc);

    for (uint32_t g0 = 0; g0 < count; g0 += G) {
        const uint32_t g = std::min(G, count - g0);
        const ZView zv{(const Fr *)d_z, z_layout, key->num_input, key->num_aux, count, g0, nvars};
        FK_HIP(ctx, hipMemcpyAsync(io + io_r, rr + (size_t)g0 * 4, (size_t)g * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        FK_HIP(ctx, hipMemcpyAsync(io + io_s, ss + (size_t)g0 * 4, (size_t)g * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        FK_TRY(evs.mark(ctx, 0));
        hipLaunchKernelGGL(batch_eval_kernel, dim3((unsigned)((m + 255) / 256), g, 3), dim3(256), 0, ctx->stream, ea, (const Fr *)r->table, zv, r->num_gates, rows, m);
        FK_HIP(ctx, hipGetLastError());
        FK_TRY(evs.mark(ctx, 1));
        if (sink) {     // a, b, c are whole and the quotient has not touched them yet; events 1 .. 9 bracket the check alone
            FK_TRY(batch_check_queue(ctx, *sink, zv, va, vb, vc, r->num_gates, m, g));
            FK_TRY(evs.mark(ctx, 9));
        }
        FK_TRY(quotient_rows(ctx, dom, va, vb, vc, g, s1, s2, vh));
        FK_TRY(evs.mark(ctx, 2));
        uint8_t *parts = io + io_parts;
        auto shape = [&](uint32_t c, uint64_t n) { return bt_msm_shape(n, c, plan.segment, g); };      // the plan's width and segment for the n points of one query
        // H: the quotient's rows, [0, m - 1)
        {
            const ScalarSrc src{ZView{vh, FK_BATCH_Z_ROWS, 0, 0, g, 0, m}, nullptr, 0};
            const BtMsmShape s = shape(plan.window_bits_g1, key->n_h);
            FK_TRY(bt_msm_front(ctx, src, (uint32_t)key->n_h, s, g, mb));
            FK_TRY(bt_msm_back<Fq>(ctx, key->d_h, s, g, mb, parts, FK_MSM_RESULT_BYTES));
        }
        FK_TRY(evs.mark(ctx, 3));
        {   // L: z at num_input + j
            const ScalarSrc src{zv, nullptr, key->num_input};
            const BtMsmShape s = shape(plan.window_bits_g1, key->n_l);
            FK_TRY(bt_msm_front(ctx, src, (uint32_t)key->n_l, s, g, mb));
            FK_TRY(bt_msm_back<Fq>(ctx, key->d_l, s, g, mb, parts + 64, FK_MSM_RESULT_BYTES));
        }
        FK_TRY(evs.mark(ctx, 4));
        {   // A: z through the A query
            const ScalarSrc src{zv, r->qidx.a, 0};
            const BtMsmShape s = shape(plan.window_bits_g1, key->n_a);
            FK_TRY(bt_msm_front(ctx, src, (uint32_t)key->n_a, s, g, mb));
            FK_TRY(bt_msm_back<Fq>(ctx, key->d_a, s, g, mb, parts + 128, FK_MSM_RESULT_BYTES));
        }
        FK_TRY(evs.mark(ctx, 5));
        {   // B1, and B2 over the same buckets where the widths agree
            const ScalarSrc src{zv, r->qidx.b, 0};
            const BtMsmShape s = shape(plan.window_bits_g1, key->n_b);
            FK_TRY(bt_msm_front(ctx, src, (uint32_t)key->n_b, s, g, mb));
            FK_TRY(bt_msm_back<Fq>(ctx, key->d_b1, s, g, mb, parts + 192, FK_MSM_RESULT_BYTES));
            FK_TRY(evs.mark(ctx, 6));
            const BtMsmShape t = shape(plan.window_bits_g2, key->n_b);
            if (t.c != s.c) FK_TRY(bt_msm_front(ctx, src, (uint32_t)key->n_b, t, g, mb));
            FK_TRY(bt_msm_back<Fq2>(ctx, key->d_b2, t, g, mb, parts + 256, FK_MSM_RESULT_BYTES));
        }
        FK_TRY(evs.mark(ctx, 7));
        hipLaunchKernelGGL(batch_assemble_kernel, dim3((g + 63) / 64), dim3(64), 0, ctx->stream, ak, (const uint8_t *)parts, (const Fr *)(io + io_r), (const Fr *)(io + io_s), g, io + io_out);
        FK_HIP(ctx, hipGetLastError());
        FK_TRY(evs.mark(ctx, 8));
        // the one place the host blocks: this group's proofs
        FK_HIP(ctx, hipMemcpyAsync(out_proofs + (size_t)g0 * FK_PROOF_BYTES, io + io_out, (size_t)g * FK_PROOF_BYTES, hipMemcpyDeviceToHost, ctx->stream));
        if (sink) FK_TRY(batch_check_download(ctx, *sink, g0, g));
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (tm) {
            double *slot[8] = {&tm->eval_ms, &tm->quotient_ms, &tm->msm_h_ms, &tm->msm_l_ms, &tm->msm_a_ms, &tm->msm_b1_ms, &tm->msm_b2_ms, &tm->assemble_ms};
            for (int i = 0; i < 8; i++) {
                float ms = 0;
                FK_HIP(ctx, hipEventElapsedTime(&ms, evs.ev[i == 1 && sink ? 9 : i], evs.ev[i + 1]));      // the quotient begins behind the check
                *slot[i] += ms;
            }
        }
        if (sink && check_ms) { float ms = 0; FK_HIP(ctx, hipEventElapsedTime(&ms, evs.ev[1], evs.ev[9])); *check_ms += ms; }
    }
    if (tm) tm->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return FK_OK;
}

}  // namespace fk

extern "C" {

int fk_prove_batch_plan(uint64_t m, uint64_t n_l, uint64_t n_a, uint64_t n_b, uint32_t count, const fk_batch_opts *opts, fk_batch_plan_info *out) {
    return fk_guard((fk_ctx *)nullptr, [&]() -> int { return bt_plan(fk::tls_error(), m, n_l, n_a, n_b, count, opts, out); });
}

int fk_prove_batch_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const void *d_z, int z_layout, uint32_t count,
                       const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_batch_dev");
    if (!ctx) return FK_ERR_BAD_ARG;
    return prove_batch_dev_impl(ctx, key, r1cs, d_z, z_layout, count, r, s, out_proofs, opts, tm);
}); }

int fk_prove_batch(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const uint64_t *z, uint32_t count,
                   const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_batch");
    if (!ctx) return FK_ERR_BAD_ARG;
    if (count == 0) { if (tm) memset(tm, 0, sizeof *tm); return FK_OK; }
    if (!key || !r1cs || !z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "fk_prove_batch: null argument");
    FK_TRY(bt_claim(ctx, "fk_prove_batch"));
    const size_t bytes = (size_t)count * ((size_t)r1cs->num_input + r1cs->num_aux) * sizeof(Fr);
    FK_HIP(ctx, ctx->bt_z.reserve(bytes));
    FK_HIP(ctx, hipMemcpyAsync(ctx->bt_z.p, z, bytes, hipMemcpyHostToDevice, ctx->stream));
    return prove_batch_dev_impl(ctx, key, r1cs, ctx->bt_z.p, FK_BATCH_Z_ROWS, count, r, s, out_proofs, opts, tm);
}); }

int fk_prove_batch_checked_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const void *d_z, int z_layout, uint32_t count,
                               const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm,
                               void *d_bad_bitmap, void *d_proof_bad, fk_check_report *reports, double *check_ms) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_batch_checked_dev");
    if (!ctx) return FK_ERR_BAD_ARG;
    const BatchCheckSink sink{(unsigned long long *)d_bad_bitmap, (uint8_t *)d_proof_bad, reports};
    return prove_batch_dev_impl(ctx, key, r1cs, d_z, z_layout, count, r, s, out_proofs, opts, tm, &sink, check_ms);
}); }

int fk_prove_batch_checked(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const uint64_t *z, uint32_t count,
                           const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm,
                           void *d_bad_bitmap, void *d_proof_bad, fk_check_report *reports, double *check_ms) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_batch_checked");
    if (!ctx) return FK_ERR_BAD_ARG;
    if (count == 0) { if (tm) memset(tm, 0, sizeof *tm); if (check_ms) *check_ms = 0; return FK_OK; }
    if (!key || !r1cs || !z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "fk_prove_batch_checked: null argument");
    if (!reports) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "fk_prove_batch_checked: null reports");
    FK_TRY(bt_claim(ctx, "fk_prove_batch_checked"));
    const size_t bytes = (size_t)count * ((size_t)r1cs->num_input + r1cs->num_aux) * sizeof(Fr);
    FK_HIP(ctx, ctx->bt_z.reserve(bytes));
    FK_HIP(ctx, hipMemcpyAsync(ctx->bt_z.p, z, bytes, hipMemcpyHostToDevice, ctx->stream));
    const BatchCheckSink sink{(unsigned long long *)d_bad_bitmap, (uint8_t *)d_proof_bad, reports};
    return prove_batch_dev_impl(ctx, key, r1cs, ctx->bt_z.p, FK_BATCH_Z_ROWS, count, r, s, out_proofs, opts, tm, &sink, check_ms);
}); }

int fk_batch_r1cs_check_dev(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, int z_layout, uint32_t count, void *d_bad_bitmap, void *d_proof_bad,
                            fk_check_report *reports, const fk_batch_opts *opts) { return fk_guard(ctx, [&]() -> int {
    const char *who = "fk_batch_r1cs_check_dev";
    FK_RANGE("fk_batch_r1cs_check_dev");
    if (!ctx) return FK_ERR_BAD_ARG;
    if (count == 0) return FK_OK;
    if (!r || !d_z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    if (!reports) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null reports", who);
    FK_TRY(bt_check_layout(ctx, z_layout, who));
    if (r->copies > 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a tiled system", who);
    FK_TRY(bt_claim(ctx, who));
    fk_batch_opts eff;
    FK_TRY(bt_budget(ctx, opts, &eff));
    const uint64_t rows = r->num_gates + r->num_input, m = (uint64_t)1 << ceil_log2_u64(rows);
    if (m >= ((uint64_t)1 << 31)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: one proof's rows do not fit 31-bit indices", who);
    // the largest group whose three rows and records fit the budget (the header states the rule); a group of one is always allowed
    const uint64_t per_proof = 3 * m * sizeof(Fr) + FK_BATCH_CHECK_RECORD_BYTES;
    const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(count, FK_BATCH_MAX_GROUP), (((uint64_t)1 << 31) - 1) / m);
    const uint32_t G = (uint32_t)std::max<uint64_t>(1, std::min(cap, eff.scratch_budget_bytes / per_proof));
    FK_HIP(ctx, ctx->bt_vec.reserve(3 * (size_t)G * m * sizeof(Fr)));
    FK_TRY(batch_check_reserve(ctx, G));
    Fr *va = ctx->bt_vec.as<Fr>(), *vb = va + (size_t)G * m, *vc = vb + (size_t)G * m;
    const BatchEvalArgs ea = bt_eval_args(r, va, vb, vc);
    const BatchCheckSink sink{(unsigned long long *)d_bad_bitmap, (uint8_t *)d_proof_bad, reports};
    for (uint32_t g0 = 0; g0 < count; g0 += G) {
        const uint32_t g = std::min(G, count - g0);
        const ZView zv{(const Fr *)d_z, z_layout, r->num_input, r->num_aux, count, g0, (uint64_t)r->num_input + r->num_aux};
        hipLaunchKernelGGL(batch_eval_kernel, dim3((unsigned)((m + 255) / 256), g, 3), dim3(256), 0, ctx->stream, ea, (const Fr *)r->table, zv, r->num_gates, rows, m);
        FK_HIP(ctx, hipGetLastError());
        FK_TRY(batch_check_queue(ctx, sink, zv, va, vb, vc, r->num_gates, m, g));
        FK_TRY(batch_check_download(ctx, sink, g0, g));
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));         // the one place the host blocks: this group's reports
    }
    return FK_OK;
}); }

int fk_batch_r1cs_eval_dev(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, int z_layout, uint32_t count, void *d_a, void *d_b, void *d_c) { return fk_guard(ctx, [&]() -> int {
    const char *who = "fk_batch_r1cs_eval_dev";
    if (!ctx) return FK_ERR_BAD_ARG;
    if (count == 0) return FK_OK;
    if (!r || !d_z || !d_a || !d_b || !d_c) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    FK_TRY(bt_check_layout(ctx, z_layout, who));
    if (r->copies > 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a tiled system", who);
    if (count > FK_BATCH_MAX_GROUP) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: more than %d proofs in one group", who, FK_BATCH_MAX_GROUP);
    FK_TRY(bt_claim(ctx, who));
    const uint64_t rows = r->num_gates + r->num_input, m = (uint64_t)1 << ceil_log2_u64(rows);
    const BatchEvalArgs ea = bt_eval_args(r, (Fr *)d_a, (Fr *)d_b, (Fr *)d_c);
    const ZView zv{(const Fr *)d_z, z_layout, r->num_input, r->num_aux, count, 0, (uint64_t)r->num_input + r->num_aux};
    hipLaunchKernelGGL(batch_eval_kernel, dim3((unsigned)((m + 255) / 256), count, 3), dim3(256), 0, ctx->stream, ea, (const Fr *)r->table, zv, r->num_gates, rows, m);
    FK_HIP(ctx, hipGetLastError());
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

int fk_batch_quotient_dev(fk_ctx *ctx, void *d_a, void *d_b, void *d_c, uint64_t n_rows, uint32_t log_m, uint32_t count, void *d_h) { return fk_guard(ctx, [&]() -> int {
    const char *who = "fk_batch_quotient_dev";
    if (!ctx) return FK_ERR_BAD_ARG;
    if (count == 0) return FK_OK;
    if (!d_a || !d_b || !d_c || !d_h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    if (log_m < 1 || log_m > FK_BATCH_MAX_LOG_M) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: domain 2^%u outside 2^1 .. 2^%d", who, log_m, FK_BATCH_MAX_LOG_M);
    const uint64_t m = (uint64_t)1 << log_m;
    if (n_rows == 0 || n_rows > m) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: %llu rows in a domain of %llu", who, (unsigned long long)n_rows, (unsigned long long)m);
    if (count > FK_BATCH_MAX_GROUP || (uint64_t)count * m >= ((uint64_t)1 << 31)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: too many proofs for one group", who);
    FK_TRY(bt_claim(ctx, who));
    NttDomain *dom = nullptr;
    FK_TRY(get_domain(ctx, log_m, &dom));
    FK_HIP(ctx, ctx->bt_vec.reserve(2 * (size_t)count * m * sizeof(Fr)));
    Fr *s1 = ctx->bt_vec.as<Fr>(), *s2 = s1 + (size_t)count * m;
    if (n_rows < m) {
        hipLaunchKernelGGL(batch_pad_kernel, dim3((unsigned)((m - n_rows + 255) / 256), count, 3), dim3(256), 0, ctx->stream, (Fr *)d_a, (Fr *)d_b, (Fr *)d_c, n_rows, m);
        FK_HIP(ctx, hipGetLastError());
    }
    FK_TRY(quotient_rows(ctx, dom, (Fr *)d_a, (Fr *)d_b, (Fr *)d_c, count, s1, s2, (Fr *)d_h));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

int fk_batch_msm_dev(fk_ctx *ctx, const void *d_bases, uint64_t n, int g2, const uint32_t *d_idx, uint32_t var_offset, const void *d_z,
                     int z_layout, uint32_t num_input, uint32_t z_vars, uint32_t count, const fk_batch_opts *opts, uint8_t *out) { return fk_guard(ctx, [&]() -> int {
    const char *who = "fk_batch_msm_dev";
    if (!ctx) return FK_ERR_BAD_ARG;
    if (count == 0) return FK_OK;
    if (!out || (n && (!d_bases || !d_z))) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    FK_TRY(bt_check_layout(ctx, z_layout, who));
    if (z_layout == FK_BATCH_Z_TILED && (num_input == 0 || num_input > z_vars)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: %u inputs of %u variables", who, num_input, z_vars);
    if (!d_idx && (uint64_t)var_offset + n > z_vars) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: variables [%u, %llu) of %u", who, var_offset, (unsigned long long)(var_offset + n), z_vars);
    if (n >= ((uint64_t)1 << 31) || count > FK_BATCH_MAX_GROUP) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: too many points or proofs for one group", who);
    uint32_t c = opts ? (g2 ? opts->window_bits_g2 : opts->window_bits_g1) : 0;
    if (c && (c < FK_BATCH_WINDOW_BITS_MIN || c > FK_BATCH_WINDOW_BITS_MAX)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: window bits %u outside %d..%d", who, c, FK_BATCH_WINDOW_BITS_MIN, FK_BATCH_WINDOW_BITS_MAX);
    FK_TRY(bt_claim(ctx, who));
    const size_t pt = g2 ? FK_G2_BYTES : FK_G1_BYTES;
    if (n == 0) { memset(out, 0, (size_t)count * pt); return FK_OK; }
    if (!c) c = bt_choose_bits(n);
    const uint32_t seg = bt_segment(n);
    if (!bt_msm_indexable(n, c, c, seg, count)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the group's buckets do not fit 31-bit indices", who);
    BtMsmBufs mb;
    FK_TRY(bt_msm_reserve(ctx, n, c, c, seg, count, &mb));
    FK_HIP(ctx, ctx->bt_io.reserve((size_t)count * pt));
    const BtMsmShape s = bt_msm_shape(n, c, seg, count);
    const ScalarSrc src{ZView{(const Fr *)d_z, z_layout, num_input, z_vars - (z_layout == FK_BATCH_Z_TILED ? num_input : 0), count, 0, z_vars}, d_idx, var_offset};
    FK_TRY(bt_msm_front(ctx, src, (uint32_t)n, s, count, mb));
    if (g2) FK_TRY(bt_msm_back<Fq2>(ctx, (const G2Affine *)d_bases, s, count, mb, ctx->bt_io.as<uint8_t>(), (uint32_t)pt));
    else FK_TRY(bt_msm_back<Fq>(ctx, (const G1Affine *)d_bases, s, count, mb, ctx->bt_io.as<uint8_t>(), (uint32_t)pt));
    FK_HIP(ctx, hipMemcpyAsync(out, ctx->bt_io.p, (size_t)count * pt, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

}  // extern "C"
