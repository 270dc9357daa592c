// The R1CS check (include/fawkes_hip_check.h): which gates a witness violates, which groups of gates (copies of a batch circuit) hold
// one, and whether the witness itself is sane (every element below r, z[0] = ONE).
//
// What the reference's debugging constraint system asserts gate by gate on the CPU (circuit/r1cs/cs.rs:157, a * b == c, "Not satisfied
// constraint") is here one multiplication and one compare per lane over the a = A z, b = B z, c = C z that r1cs_eval_impl (spmv.hip)
// leaves in the context's stage buffers -- every form of the resident system (plain, length-class lists, tiled wave kernel, alias rows)
// is covered by the evaluator the prover uses, and inside a proof the check reads the very vectors the quotient is made from.
//
// Kernels, all on the library's stream:
//   check_init_kernel      the counters
//   check_range_kernel     one witness element per lane against r; count and lowest index; z[0] against ONE
//   check_gates_kernel     one gate per lane; the wave's ballot word IS the bitmap word; count and lowest index per wave
//   check_groups_kernel    how many group flags are set
//   check_first_kernel     a, b, c of the lowest bad gate into the counters (inside a proof the stage buffers do not outlive the quotient)
// The gate kernel streams 96 bytes per gate and writes one bit: it is bound by HBM reads.
#include "common.hpp"
#include <string.h>

#include "r1cs.hpp"
#include "check_shared.hpp"
#include "../../include/fawkes_hip_check.h"

namespace fk {

// device-side record of one check; the head of ctx->check
struct CheckCounters {
    unsigned long long n_bad, first_bad, n_bad_groups, n_range, first_range;
    uint32_t one_ok, pad;
    Fr abc[3];
};
static constexpr size_t CHECK_HEAD = 256;
static_assert(sizeof(CheckCounters) <= CHECK_HEAD, "the counters fit the head of the scratch");

__global__ void check_init_kernel(CheckCounters *cnt) {
    if (blockIdx.x || threadIdx.x) return;
    cnt->n_bad = 0; cnt->first_bad = CHECK_NONE; cnt->n_bad_groups = 0; cnt->n_range = 0; cnt->first_range = CHECK_NONE;
    cnt->one_ok = 0; cnt->pad = 0;
    for (int k = 0; k < 3; k++) cnt->abc[k] = Fr::zero();
}

// One witness element per lane.  The count and the lowest index are reduced per wave (the ballot), then one atomic add and one atomic
// min per wave THAT HOLDS an element not below r: a witness in range issues none.
__global__ __launch_bounds__(256) void check_range_kernel(const Fr *z, uint64_t n, CheckCounters *cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool out = false;
    if (i < n) {
        const Fr x = z[i];
        out = !image_below_r(x);
        if (i == 0) cnt->one_ok = x == Fr::one() ? 1u : 0u;
    }
    const unsigned long long word = __ballot(out);
    if (word && (threadIdx.x & 63) == 0) {
        atomicAdd(&cnt->n_range, (unsigned long long)__popcll(word));
        atomicMin(&cnt->first_range, (unsigned long long)(i + (uint64_t)(__ffsll((long long)word) - 1)));
    }
}

// One gate per lane: product_differs (check_shared.hpp).  A block is four waves of 64 consecutive gates, so lane 0 of a wave sits on gate
// 64 * w and the wave's ballot is word w of the bitmap: one ordinary vector store from that lane, and the lanes behind the last gate
// contribute zero bits.  n_bad and first_bad: popcount and lowest set bit of the ballot, one atomic add and one atomic min per wave
// that has a bad gate -- a satisfied system issues no atomic at all.  Group flags: a bad lane stores 1 into its group's byte (zeroed
// before the launch); the stores to one byte all carry the same value, and only bad lanes pay the division.
// Reads: 3 x 32 bytes per lane, consecutive lanes on consecutive elements (two 16-byte loads per element, 2 KB contiguous per wave
// and array).
__global__ __launch_bounds__(256) void check_gates_kernel(const Fr *a, const Fr *b, const Fr *c, uint64_t gates, uint64_t group_rows,
                                                           unsigned long long *bitmap, uint8_t *group_bad, CheckCounters *cnt) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (g < gates) bad = product_differs(a[g], b[g], c[g]);
    const unsigned long long word = __ballot(bad);
    if (bad && group_bad) group_bad[g / group_rows] = 1;
    if ((threadIdx.x & 63) == 0 && g < gates) {
        bitmap[g >> 6] = word;
        if (word) {
            atomicAdd(&cnt->n_bad, (unsigned long long)__popcll(word));
            atomicMin(&cnt->first_bad, (unsigned long long)(g + (uint64_t)(__ffsll((long long)word) - 1)));
        }
    }
}

__global__ __launch_bounds__(256) void check_groups_kernel(const uint8_t *group_bad, uint64_t n_groups, CheckCounters *cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long word = __ballot(k < n_groups && group_bad[k] != 0);
    if (word && (threadIdx.x & 63) == 0) atomicAdd(&cnt->n_bad_groups, (unsigned long long)__popcll(word));
}

__global__ void check_first_kernel(const Fr *a, const Fr *b, const Fr *c, CheckCounters *cnt) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long g = cnt->first_bad;
    if (g == CHECK_NONE) return;
    cnt->abc[0] = a[g]; cnt->abc[1] = b[g]; cnt->abc[2] = c[g];
}

// What one check writes and where.  bitmap / flags: the caller's device arrays, or the context's scratch behind the counters.
struct CheckPlan {
    uint64_t gates = 0, words = 0, group_rows = 0, n_groups = 0, n_vars = 0;
    CheckCounters *cnt = nullptr;
    unsigned long long *bitmap = nullptr;
    uint8_t *flags = nullptr;
};

static int check_args(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, uint64_t group_rows, const void *d_group_bad, const fk_check_report *report) {
    if (!r || !d_z || !report) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: null argument");
    if (d_group_bad && !group_rows) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: group flags asked for with group_rows = 0");
    return FK_OK;
}

// sizes the scratch (grow-only, possibly a reallocation: before anything of this call is queued)
static int check_plan(fk_ctx *ctx, const fk_r1cs_dev *r, uint64_t group_rows, void *d_bad_bitmap, void *d_group_bad, CheckPlan *p) {
    p->gates = r->num_gates;
    p->words = (p->gates + 63) / 64;
    p->group_rows = group_rows;
    p->n_groups = group_rows ? (p->gates + group_rows - 1) / group_rows : 0;
    p->n_vars = (uint64_t)r->num_input + r->num_aux;
    const size_t own_words = d_bad_bitmap ? 0 : p->words, own_flags = d_group_bad ? 0 : p->n_groups;
    FK_HIP(ctx, ctx->check.reserve(CHECK_HEAD + own_words * 8 + own_flags));
    uint8_t *base = ctx->check.as<uint8_t>();
    p->cnt = (CheckCounters *)base;
    p->bitmap = d_bad_bitmap ? (unsigned long long *)d_bad_bitmap : (unsigned long long *)(base + CHECK_HEAD);
    p->flags = !group_rows ? nullptr : (d_group_bad ? (uint8_t *)d_group_bad : base + CHECK_HEAD + own_words * 8);
    return FK_OK;
}

static int check_queue_range(fk_ctx *ctx, const CheckPlan &p, const void *d_z) {
    hipLaunchKernelGGL(check_init_kernel, dim3(1), dim3(64), 0, ctx->stream, p.cnt);
    if (p.n_vars) hipLaunchKernelGGL(check_range_kernel, dim3((unsigned)((p.n_vars + 255) / 256)), dim3(256), 0, ctx->stream, (const Fr *)d_z, p.n_vars, p.cnt);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "check_range");
    return FK_OK;
}

// a, b, c: the evaluated rows (at least p.gates elements each), complete at this point of the stream
static int check_queue_gates(fk_ctx *ctx, const CheckPlan &p, const void *d_a, const void *d_b, const void *d_c) {
    const Fr *a = (const Fr *)d_a, *b = (const Fr *)d_b, *c = (const Fr *)d_c;
    if (p.flags && p.n_groups) FK_HIP(ctx, hipMemsetAsync(p.flags, 0, p.n_groups, ctx->stream));
    if (p.gates) {
        if ((p.gates + 255) / 256 > 0x7fffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: system too large for one launch");
        hipLaunchKernelGGL(check_gates_kernel, dim3((unsigned)((p.gates + 255) / 256)), dim3(256), 0, ctx->stream, a, b, c, p.gates, p.group_rows, p.bitmap, p.flags, p.cnt);
        if (p.n_groups) hipLaunchKernelGGL(check_groups_kernel, dim3((unsigned)((p.n_groups + 255) / 256)), dim3(256), 0, ctx->stream, p.flags, p.n_groups, p.cnt);
        hipLaunchKernelGGL(check_first_kernel, dim3(1), dim3(64), 0, ctx->stream, a, b, c, p.cnt);
    }
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "check_gates");
    return FK_OK;
}

// waits for the stream and turns the counters into the report
static int check_collect(fk_ctx *ctx, const CheckPlan &p, fk_check_report *rep) {
    CheckCounters h;
    FK_HIP(ctx, hipMemcpyAsync(&h, p.cnt, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memset(rep, 0, sizeof *rep);
    rep->gates = p.gates;
    rep->n_bad = h.n_bad; rep->first_bad = h.first_bad;
    memcpy(rep->first_abc, h.abc, sizeof rep->first_abc);
    rep->n_groups = p.n_groups; rep->n_bad_groups = h.n_bad_groups;
    rep->n_range = h.n_range; rep->first_range = h.first_range;
    rep->one_ok = (int32_t)h.one_ok;
    rep->gates_valid = h.n_range == 0;
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

static_assert(sizeof(fk_check_report) == 160, "fk_check_report has no padding");
static_assert(FK_CHECK_NONE == CHECK_NONE, "one sentinel");

// The host reference: plain C++ over the CSR with the arithmetic of fk_synthesize (a unit coefficient is not multiplied, the terms are
// added in row order).  Copy j of a tiled system is walked by the index arithmetic fk_r1cs_load_tiled documents -- ONE shared, then
// every copy's inputs, then every copy's aux -- and the replicated system is never materialised.
static int r1cs_check_host(fk_ctx *ctx, const fk_r1cs *cs, uint32_t copies, const uint64_t *z_, uint64_t group_rows, uint64_t *bad_bitmap,
                           uint8_t *group_bad, fk_check_report *rep) {
    if (!cs || !z_ || !rep) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: null argument");
    if (!copies) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: copies = 0");
    if (group_bad && !group_rows) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: group flags asked for with group_rows = 0");
    CsrView mats[3];
    FK_TRY(check_host_system(ctx, cs, mats));
    const uint64_t G = cs->num_gates, gates = G * copies;
    const uint64_t num_input = 1 + (uint64_t)copies * (cs->num_input - 1), n_vars = num_input + (uint64_t)copies * cs->num_aux;
    if (n_vars > 0xffffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: the batch does not fit 32-bit variable indices");
    const uint64_t words = (gates + 63) / 64, n_groups = group_rows ? (gates + group_rows - 1) / group_rows : 0;
    memset(rep, 0, sizeof *rep);
    if (bad_bitmap) memset(bad_bitmap, 0, words * 8);
    if (group_bad) memset(group_bad, 0, n_groups);
    rep->gates = gates; rep->n_groups = n_groups;
    rep->first_bad = rep->first_range = FK_CHECK_NONE;
    const Fr *z = (const Fr *)z_;
    const Fr one = Fr::one();
    for (uint64_t i = 0; i < n_vars; i++)
        if (!image_below_r(z[i])) { if (!rep->n_range++) rep->first_range = i; }
    rep->one_ok = z[0] == one;
    rep->gates_valid = rep->n_range == 0;
    if (!rep->gates_valid) return FK_OK;        // the gate fields are unspecified: left at "none", the arrays zeroed
    uint64_t last_group = FK_CHECK_NONE;
    for (uint32_t copy = 0; copy < copies; copy++) {
        // instance variable v != 0 of this copy: an input moves by in_off, an aux variable by aux_off
        const uint64_t in_off = (uint64_t)copy * (cs->num_input - 1), aux_off = num_input + (uint64_t)copy * cs->num_aux - cs->num_input;
        for (uint64_t row = 0; row < G; row++) {
            Fr abc[3];
            for (int m = 0; m < 3; m++)
                abc[m] = csr_row_dot(mats[m], row, z, [&](uint64_t v) { return v ? v + (v < cs->num_input ? in_off : aux_off) : 0; });
            if (!product_differs(abc[0], abc[1], abc[2])) continue;
            const uint64_t g = (uint64_t)copy * G + row;
            if (!rep->n_bad++) { rep->first_bad = g; memcpy(rep->first_abc, abc, sizeof rep->first_abc); }
            if (bad_bitmap) bad_bitmap[g >> 6] |= (uint64_t)1 << (g & 63);
            if (group_rows && g / group_rows != last_group) {           // gates come in ascending order: a group is counted at its first bad gate
                last_group = g / group_rows;
                rep->n_bad_groups++;
                if (group_bad) group_bad[last_group] = 1;
            }
        }
    }
    return FK_OK;
}

int fk_r1cs_check(fk_ctx *ctx, const fk_r1cs *cs, uint32_t copies, const uint64_t *z, uint64_t group_rows, uint64_t *bad_bitmap,
                  uint8_t *group_bad, fk_check_report *rep) { return fk_guard(ctx, [&]() -> int {
    if (ctx) return r1cs_check_host(ctx, cs, copies, z, group_rows, bad_bitmap, group_bad, rep);
    fk_ctx local;                  // host-only routine: usable without a GPU context; its message goes where fk_last_error(NULL) reads
    const int rc = r1cs_check_host(&local, cs, copies, z, group_rows, bad_bitmap, group_bad, rep);
    if (rc != FK_OK) tls_error() = local.err;
    return rc;
}); }

int fk_r1cs_check_dev(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, uint64_t group_rows, void *d_bad_bitmap, void *d_group_bad,
                      fk_check_report *rep) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_r1cs_check_dev");
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(check_args(ctx, r, d_z, group_rows, d_group_bad, rep));
    FK_TRY(scratch_claim(ctx, "check"));      // the stage buffers may hold the a, b, c of a submitted proof whose front ran early
    CheckPlan p;
    FK_TRY(check_plan(ctx, r, group_rows, d_bad_bitmap, d_group_bad, &p));
    const size_t rb = ((size_t)r->num_gates + r->num_input) * sizeof(Fr);
    FK_HIP(ctx, ctx->stage_a.reserve(rb)); FK_HIP(ctx, ctx->stage_b.reserve(rb)); FK_HIP(ctx, ctx->stage_c.reserve(rb));
    FK_TRY(check_queue_range(ctx, p, d_z));
    FK_TRY(r1cs_eval_impl(ctx, r, d_z, ctx->stage_a.p, ctx->stage_b.p, ctx->stage_c.p, false, 0, 0, 0, -1));
    FK_TRY(check_queue_gates(ctx, p, ctx->stage_a.p, ctx->stage_b.p, ctx->stage_c.p));
    return check_collect(ctx, p, rep);
}); }

int fk_prove_r1cs_checked_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_z, const uint64_t rr[4], const uint64_t ss[4],
                              uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm, uint64_t group_rows, void *d_bad_bitmap, void *d_group_bad,
                              fk_check_report *rep) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_r1cs_checked_dev");
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!key) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: null argument");
    FK_TRY(check_args(ctx, r, d_z, group_rows, d_group_bad, rep));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    CheckPlan p;
    FK_TRY(check_plan(ctx, r, group_rows, d_bad_bitmap, d_group_bad, &p));      // may reallocate the scratch: before anything is queued
    bool queued = false;
    // Everything of the check is queued behind the evaluation, the range kernel included: in front of it it would stand between the
    // witness and the event the witness multiplications wait for.
    const std::function<int()> after_eval = [&]() -> int {
        FK_TRY(check_queue_range(ctx, p, d_z));
        FK_TRY(check_queue_gates(ctx, p, ctx->stage_a.p, ctx->stage_b.p, ctx->stage_c.p));
        queued = true;
        return FK_OK;
    };
    const int rc = prove_r1cs_dev_impl(ctx, key, r, d_z, rr, ss, out_proof, tm, &after_eval, nullptr);
    if (rc != FK_OK) {
        if (queued) (void)hipStreamSynchronize(ctx->stream);        // the caller's arrays are no longer written when an error returns
        return rc;
    }
    return check_collect(ctx, p, rep);
}); }

}  // extern "C"
