// The batch prover's R1CS check (include/fawkes_hip_batch_check.h): one verdict per proof of a group, over the a = A z, b = B z, c = C z
// that batch_eval_kernel (batch_prove.hip) leaves proof-major in ctx->bt_vec -- check.hip's kernels with the proof index as gridDim.y,
// one record per proof instead of one per call.  The predicates are check.hip's (check_shared.hpp), the place of a variable is the
// batch prover's (batch_shared.hpp: zaddr).
//
// Kernels, all on the library's stream, FK_BATCH_CHECK_LAUNCHES per group:
//   batch_check_init_kernel     the records: one lane per proof
//   batch_check_range_kernel    one (variable, proof) per lane against r; count and lowest variable per proof; z[0] against ONE
//   batch_check_gates_kernel    one (gate, proof) per lane; the wave's ballot IS a word of the proof's bitmap
//   batch_check_close_kernel    one lane per proof: a, b, c of its lowest bad gate (the rows do not outlive the quotient), its flag
// The device record IS fk_check_report, so a group's reports come down in one copy.  The gate kernel streams 96 bytes per lane and
// writes one bit: bound by HBM reads.
#include "common.hpp"
#include <string.h>
#include <stddef.h>

#include "check_shared.hpp"
#include "batch_shared.hpp"

namespace fk {

// fk_check_report with the counters as the types the device atomics take (abc: limbs, an Fr is aligned to 16 bytes and offset 24 is not)
struct BatchCheckRec {
    unsigned long long gates, n_bad, first_bad;
    uint32_t abc[3][8];
    unsigned long long n_groups, n_bad_groups, n_range, first_range;
    int32_t one_ok, gates_valid;
};
static_assert(sizeof(BatchCheckRec) == sizeof(fk_check_report) && sizeof(BatchCheckRec) == FK_BATCH_CHECK_RECORD_BYTES, "the device record is the report");
static_assert(offsetof(BatchCheckRec, abc) == offsetof(fk_check_report, first_abc) && offsetof(BatchCheckRec, n_range) == offsetof(fk_check_report, n_range)
              && offsetof(BatchCheckRec, one_ok) == offsetof(fk_check_report, one_ok), "the device record is the report");
static_assert(FK_CHECK_NONE == CHECK_NONE, "one sentinel");

__global__ __launch_bounds__(64) void batch_check_init_kernel(BatchCheckRec *rec, uint32_t proofs, uint64_t gates) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= proofs) return;
    BatchCheckRec r;
    r.gates = gates; r.n_bad = 0; r.first_bad = CHECK_NONE;
    for (int k = 0; k < 3; k++) for (int l = 0; l < 8; l++) r.abc[k][l] = 0;
    r.n_groups = 0; r.n_bad_groups = 0; r.n_range = 0; r.first_range = CHECK_NONE;
    r.one_ok = 0; r.gates_valid = 0;
    rec[p] = r;
}

// Grid (ceil(nvars / 256), proofs): lane (v, p) holds variable v of proof p, wherever the layout keeps it -- under FK_BATCH_Z_TILED every
// proof's lane 0 reads the one shared ONE.  Per proof what check_range_kernel does per call: the ballot, then one atomic add and one
// atomic min per wave THAT HOLDS an element not below r.
__global__ __launch_bounds__(256) void batch_check_range_kernel(ZView zv, uint32_t nvars, BatchCheckRec *rec) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    bool out = false;
    if (v < nvars) {
        const Fr x = zv.z[zaddr(zv, p, v)];
        out = !image_below_r(x);
        if (v == 0) rec[p].one_ok = x == Fr::one() ? 1 : 0;
    }
    const unsigned long long word = __ballot(out);
    if (word && (threadIdx.x & 63) == 0) {
        atomicAdd(&rec[p].n_range, (unsigned long long)__popcll(word));
        atomicMin(&rec[p].first_range, (unsigned long long)(v + (uint32_t)(__ffsll((long long)word) - 1)));
    }
}

// Grid (ceil(gates / 256), proofs): lane (t, p) reads a, b, c at p * m + t.  A block starts at t = 0 of its proof, so lane 0 of a wave
// sits on a multiple of 64 and the wave's ballot is word p * words + (t >> 6) of the bitmap: one ordinary vector store from that lane,
// the lanes behind the last gate contribute zero bits.  n_bad and first_bad of the proof: one atomic add and one atomic min per wave
// that HAS a bad gate -- a satisfied batch issues none.  A proof with an element not below r (the range kernel ran before this one) is
// not judged: the load is uniform over the block, its words are written as zeros.
// Reads: 3 x 32 bytes per lane, consecutive lanes on consecutive elements, as in check_gates_kernel.
__global__ __launch_bounds__(256) void batch_check_gates_kernel(const Fr *a, const Fr *b, const Fr *c, uint64_t gates, uint64_t m, uint64_t words,
                                                                 unsigned long long *bitmap, BatchCheckRec *rec) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t p = blockIdx.y;
    bool bad = false;
    if (t < gates && rec[p].n_range == 0) {
        const uint64_t i = (uint64_t)p * m + t;
        bad = product_differs(a[i], b[i], c[i]);
    }
    const unsigned long long word = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && t < gates) {
        if (bitmap) bitmap[(uint64_t)p * words + (t >> 6)] = word;
        if (word) {
            atomicAdd(&rec[p].n_bad, (unsigned long long)__popcll(word));
            atomicMin(&rec[p].first_bad, (unsigned long long)(t + (uint64_t)(__ffsll((long long)word) - 1)));
        }
    }
}

__global__ __launch_bounds__(64) void batch_check_close_kernel(const Fr *a, const Fr *b, const Fr *c, uint64_t m, uint32_t proofs, BatchCheckRec *rec, uint8_t *proof_bad) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= proofs) return;
    const unsigned long long g = rec[p].first_bad, n_range = rec[p].n_range;
    if (g != CHECK_NONE) {
        const uint64_t i = (uint64_t)p * m + g;
        const Fr x[3] = {a[i], b[i], c[i]};
        for (int k = 0; k < 3; k++) for (int l = 0; l < 8; l++) rec[p].abc[k][l] = x[k].v[l];
    }
    rec[p].gates_valid = n_range == 0;
    if (proof_bad) proof_bad[p] = (rec[p].n_bad > 0 || n_range > 0 || !rec[p].one_ok) ? 1 : 0;
}

int batch_check_reserve(fk_ctx *ctx, uint32_t group) {
    FK_HIP(ctx, ctx->bt_check.reserve((size_t)group * sizeof(BatchCheckRec)));
    return FK_OK;
}

int batch_check_queue(fk_ctx *ctx, const BatchCheckSink &sink, const ZView &zv, const Fr *a, const Fr *b, const Fr *c, uint64_t gates, uint64_t m, uint32_t g) {
    BatchCheckRec *rec = ctx->bt_check.as<BatchCheckRec>();
    const uint32_t nvars = zv.num_input + zv.num_aux;
    const uint64_t words = (gates + 63) / 64;
    hipLaunchKernelGGL(batch_check_init_kernel, dim3((g + 63) / 64), dim3(64), 0, ctx->stream, rec, g, gates);
    hipLaunchKernelGGL(batch_check_range_kernel, dim3((nvars + 255) / 256, g), dim3(256), 0, ctx->stream, zv, nvars, rec);
    if (gates)
        hipLaunchKernelGGL(batch_check_gates_kernel, dim3((unsigned)((gates + 255) / 256), g), dim3(256), 0, ctx->stream, a, b, c, gates, m, words,
                           sink.d_bitmap ? sink.d_bitmap + (size_t)zv.p0 * words : nullptr, rec);
    hipLaunchKernelGGL(batch_check_close_kernel, dim3((g + 63) / 64), dim3(64), 0, ctx->stream, a, b, c, m, g, rec, sink.d_proof_bad ? sink.d_proof_bad + zv.p0 : nullptr);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "batch_check");
    return FK_OK;
}

int batch_check_download(fk_ctx *ctx, const BatchCheckSink &sink, uint32_t p0, uint32_t g) {
    FK_HIP(ctx, hipMemcpyAsync(sink.reports + p0, ctx->bt_check.p, (size_t)g * sizeof(BatchCheckRec), hipMemcpyDeviceToHost, ctx->stream));
    return FK_OK;
}

// The host reference: plain C++ over the CSR of ONE instance with the arithmetic of fk_synthesize (csr_row_dot); variable v of proof i
// is found by zaddr, the rule the device stages read z by.
static int batch_check_host(fk_ctx *ctx, const fk_r1cs *cs, const uint64_t *z_, int z_layout, uint32_t count, uint64_t *bad_bitmap, uint8_t *proof_bad,
                            fk_check_report *reports) {
    if (count == 0) return FK_OK;
    if (!cs || !z_ || !reports) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "fk_batch_r1cs_check: null argument");
    if (z_layout != FK_BATCH_Z_ROWS && z_layout != FK_BATCH_Z_TILED) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "fk_batch_r1cs_check: unknown witness layout %d", z_layout);
    CsrView mats[3];
    FK_TRY(check_host_system(ctx, cs, mats));
    const uint64_t G = cs->num_gates, words = (G + 63) / 64;
    const uint32_t nvars = cs->num_input + cs->num_aux;
    const Fr *z = (const Fr *)z_;
    const ZView zv{z, z_layout, cs->num_input, cs->num_aux, count, 0, nvars};
    const Fr one = Fr::one();
    for (uint32_t i = 0; i < count; i++) {
        fk_check_report *rep = reports + i;
        uint64_t *bitmap = bad_bitmap ? bad_bitmap + (size_t)i * words : nullptr;
        memset(rep, 0, sizeof *rep);
        if (bitmap) memset(bitmap, 0, words * 8);
        rep->gates = G;
        rep->first_bad = rep->first_range = FK_CHECK_NONE;
        for (uint32_t v = 0; v < nvars; v++)
            if (!image_below_r(z[zaddr(zv, i, v)])) { if (!rep->n_range++) rep->first_range = v; }
        rep->one_ok = z[zaddr(zv, i, 0)] == one;
        rep->gates_valid = rep->n_range == 0;
        for (uint64_t row = 0; row < G && rep->gates_valid; row++) {
            Fr abc[3];
            for (int m = 0; m < 3; m++) abc[m] = csr_row_dot(mats[m], row, z, [&](uint32_t v) { return zaddr(zv, i, v); });
            if (!product_differs(abc[0], abc[1], abc[2])) continue;
            if (!rep->n_bad++) { rep->first_bad = row; memcpy(rep->first_abc, abc, sizeof rep->first_abc); }
            if (bitmap) bitmap[row >> 6] |= (uint64_t)1 << (row & 63);
        }
        if (proof_bad) proof_bad[i] = (rep->n_bad > 0 || rep->n_range > 0 || !rep->one_ok) ? 1 : 0;
    }
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_batch_r1cs_check(fk_ctx *ctx, const fk_r1cs *cs, const uint64_t *z, int z_layout, uint32_t count, uint64_t *bad_bitmap, uint8_t *proof_bad,
                        fk_check_report *reports) { return fk_guard(ctx, [&]() -> int {
    if (ctx) return batch_check_host(ctx, cs, z, z_layout, count, bad_bitmap, proof_bad, reports);
    fk_ctx local;                  // host-only routine: usable without a GPU context; its message goes where fk_last_error(NULL) reads
    const int rc = batch_check_host(&local, cs, z, z_layout, count, bad_bitmap, proof_bad, reports);
    if (rc != FK_OK) tls_error() = local.err;
    return rc;
}); }

}  // extern "C"
