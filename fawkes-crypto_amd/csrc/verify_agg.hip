// Aggregated batch verification (include/fawkes_hip_verify.h): `count` Groth16 proofs of one key, ONE pairing equation.
//
// With secret nonzero 128-bit weights w_i the count equations of verify.hip hold, except with probability ~2^-128, iff
//     prod_i e(w_i A_i, B_i) * e(-(sum w_i) alpha, beta) * e(-S_acc, gamma) * e(-S_C, delta) = 1,
//     S_C = sum w_i C_i,  S_acc = (sum w_i) ic_0 + sum_j (sum_i w_i x_ij) ic_j.
// Per proof: the pre-checks of verify_one (the subgroup check of B among them), two 128-bit G1 multiplications and one Miller loop
// (pairing.hpp: miller_loop_proj).  Per batch: the sums in Fr, n_ic + 1 scalar multiplications, three Miller loops and the final
// exponentiation -- on the host, a fixed cost of some milliseconds, deliberately not moved to the device here.
//
// Device: one proof per lane, 64 lanes per workgroup, FqC (out-of-line multiply) like verify_batch_kernel.  Four kernels, so that
// each one's registers are set by what it needs: agg_prepare_kernel (decode, checks, w A, w C), agg_miller_kernel (f_i), and one launch
// per level of f12_level_kernel / g1_level_kernel down to the product of the f_i and the sum of the w_i C_i (the shape of
// poseidon_level_kernel; a fused tail was measured there and dropped).  The host entry runs the same templates on the CPU.
#include "verify_decode.hpp"
#include "poseidon.hpp"          // chacha20_block
#include "../../include/fawkes_hip_verify.h"
#include <sys/random.h>
#include <errno.h>

namespace fk {

// The Miller loop of the aggregate path.  -DFK_VERIFY_AGG_AFFINE: the affine loop of the per-proof verifier, for the A/B measurement of
// tools/verify_bench.py only (the two differ by factors the final exponentiation kills, so either is correct; not a shipped mode).
template <class Fq>
static FK_HD Fq12T<Fq> agg_miller(const Affine<Fq> &P, const Affine<Fq2T<Fq>> &Q) {
#ifdef FK_VERIFY_AGG_AFFINE
    return miller_loop<Fq>(P, Q);
#else
    return miller_loop_proj<Fq>(P, Q);
#endif
}

// One proof: decode, the well-formedness checks of verify_one (for the reason given there: the Miller loop assumes a B of prime order
// r), then w A (affine: miller_loop_proj says why) and w C.  A proof that is not well-formed leaves three identities behind, so its
// Miller value is one and it adds nothing to S_C.
template <class Fq>
static FK_HD bool agg_prepare_one(const uint8_t *proof, uint64_t w_lo, uint64_t w_hi, Affine<Fq> &wA, Affine<Fq2T<Fq>> &B, Xyzz<Fq> &wC) {
    using F2 = Fq2T<Fq>;
    bool ok = true;
    const Affine<Fq> A = g1_from_borsh<Fq>(proof, &ok), C = g1_from_borsh<Fq>(proof + 192, &ok);
    B = g2_from_borsh<Fq>(proof + 64, &ok);
    if (ok) {
        const uint32_t bw[8] = FK_G1_B, b0[8] = FK_G2_B0, b1[8] = FK_G2_B1, rw[8] = FK_R_CANON;
        auto cst = [](const uint32_t (&w)[8]) { Fq t; for (int i = 0; i < 8; i++) t.v[i] = w[i]; return t; };
        auto on_g1 = [&](const Affine<Fq> &P) { return P.is_inf() || Fq::sqr(P.y) == Fq::add(Fq::mul(Fq::sqr(P.x), P.x), cst(bw)); };
        ok = on_g1(A) && on_g1(C);
        if (ok && !B.is_inf()) {
            ok = F2::sqr(B.y) == F2::add(F2::mul(F2::sqr(B.x), B.x), F2{cst(b0), cst(b1)});
            if (ok) ok = Xyzz<F2>::mul_scalar(Xyzz<F2>::from_affine(B), rw).is_inf();
        }
    }
    if (!ok) { wA = Affine<Fq>::inf(); B = Affine<F2>::inf(); wC = Xyzz<Fq>::inf(); return false; }
    wA = Xyzz<Fq>::mul_affine_bits(A, w_lo, w_hi, 128).to_affine();
    wC = Xyzz<Fq>::mul_affine_bits(C, w_lo, w_hi, 128);
    return true;
}

using G1C = Xyzz<FqC>;
using F12C = Fq12T<FqC>;

__global__ __launch_bounds__(64) void agg_prepare_kernel(const uint8_t *__restrict__ proofs, const uint64_t *__restrict__ weights, uint32_t count,
                                                         Affine<FqC> *__restrict__ wa, Affine<Fq2C> *__restrict__ b, G1C *__restrict__ wc, uint8_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Affine<FqC> wA; Affine<Fq2C> B; G1C wC;
    flag[i] = agg_prepare_one<FqC>(proofs + (size_t)i * FK_PROOF_BYTES, weights[2 * (size_t)i], weights[2 * (size_t)i + 1], wA, B, wC) ? 1 : 0;
    wa[i] = wA; b[i] = B; wc[i] = wC;
}

__global__ __launch_bounds__(64) void agg_miller_kernel(const Affine<FqC> *__restrict__ wa, const Affine<Fq2C> *__restrict__ b, uint32_t count, F12C *__restrict__ f) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    f[i] = agg_miller<FqC>(wa[i], b[i]);           // an identity operand (a flagged proof) gives one
}

// one level of the product / sum tree: out[i] = in[2 i] (op) in[2 i + 1], an odd last element is carried over; n_out = ceil(n_in / 2)
__global__ __launch_bounds__(64) void f12_level_kernel(const F12C *__restrict__ in, uint32_t n_in, F12C *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * (uint64_t)i >= n_in) return;
    out[i] = 2 * (uint64_t)i + 1 < n_in ? F12C::mul(in[2 * (size_t)i], in[2 * (size_t)i + 1]) : in[2 * (size_t)i];
}
__global__ __launch_bounds__(64) void g1_level_kernel(const G1C *__restrict__ in, uint32_t n_in, G1C *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * (uint64_t)i >= n_in) return;
    G1C a = in[2 * (size_t)i];
    if (2 * (uint64_t)i + 1 < n_in) a.add(in[2 * (size_t)i + 1]);
    out[i] = a;
}

// elements of all levels of a tree over n leaves, the leaves included: n + ceil(n / 2) + ... + 1
static size_t level_total(uint32_t n) {
    size_t t = n;
    while (n > 1) { n = (n + 1) / 2; t += n; }
    return t;
}

// count x 2 u64 from a ChaCha20 stream keyed with 32 bytes of the kernel's entropy; a zero draw is redrawn
static int draw_weights(fk_ctx *ctx, uint32_t count, std::vector<uint64_t> &w) {
    uint32_t key[8];
    size_t got = 0;
    while (got < sizeof key) {
        const ssize_t r = getrandom((uint8_t *)key + got, sizeof key - got, 0);
        if (r < 0) { if (errno == EINTR) continue; FK_SET_ERR(ctx, FK_ERR_UNSUPPORTED, "verify_aggregate: getrandom failed (errno %d): no weights can be drawn", errno); }
        got += (size_t)r;
    }
    w.resize((size_t)count * 2);
    uint32_t blk[16]; int pos = 16; uint64_t counter = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t lo, hi;
        do {
            if (pos >= 16) { chacha20_block(key, counter++, 0, blk); pos = 0; }
            lo = (uint64_t)blk[pos] | (uint64_t)blk[pos + 1] << 32; hi = (uint64_t)blk[pos + 2] | (uint64_t)blk[pos + 3] << 32;
            pos += 4;
        } while (!(lo | hi));
        w[2 * (size_t)i] = lo; w[2 * (size_t)i + 1] = hi;
    }
    return FK_OK;
}

// what the per-proof stage (host loop or kernels) hands to the tail
struct AggFront {
    std::vector<uint8_t> flag;
    Fq12T<Fq> f = Fq12T<Fq>::one();     // product of the Miller values
    Xyzz<Fq> s_c = Xyzz<Fq>::inf();     // sum of w_i C_i
};

static int front_host(const uint8_t *proofs, uint32_t count, const uint64_t *w, AggFront &o) {
    for (uint32_t i = 0; i < count; i++) {
        Affine<Fq> wA; Affine<Fq2> B; Xyzz<Fq> wC;
        o.flag[i] = agg_prepare_one<Fq>(proofs + (size_t)i * FK_PROOF_BYTES, w[2 * (size_t)i], w[2 * (size_t)i + 1], wA, B, wC) ? 1 : 0;
        if (!o.flag[i]) continue;
        o.f = Fq12T<Fq>::mul(o.f, agg_miller<Fq>(wA, B));
        o.s_c.add(wC);
    }
    return FK_OK;
}

static int front_dev(fk_ctx *ctx, const uint8_t *proofs, uint32_t count, const uint64_t *w, AggFront &o) {
    FK_TRY(scratch_claim(ctx, "verify_aggregate"));
    const size_t pr_b = (size_t)count * FK_PROOF_BYTES, w_b = (size_t)count * 16, lev = level_total(count);
    FK_HIP(ctx, ctx->misc.reserve(pr_b + w_b));
    FK_HIP(ctx, ctx->stage_a.reserve((size_t)count * sizeof(Affine<FqC>)));
    FK_HIP(ctx, ctx->stage_b.reserve((size_t)count * sizeof(Affine<Fq2C>)));
    FK_HIP(ctx, ctx->stage_c.reserve(lev * sizeof(G1C)));
    FK_HIP(ctx, ctx->stage_z.reserve(lev * sizeof(F12C)));
    FK_HIP(ctx, ctx->stage_d.reserve(count));
    uint8_t *d_pr = ctx->misc.as<uint8_t>();
    uint64_t *d_w = (uint64_t *)(d_pr + pr_b);
    Affine<FqC> *d_wa = ctx->stage_a.as<Affine<FqC>>();
    Affine<Fq2C> *d_b = ctx->stage_b.as<Affine<Fq2C>>();
    G1C *d_wc = ctx->stage_c.as<G1C>();
    F12C *d_f = ctx->stage_z.as<F12C>();
    uint8_t *d_flag = ctx->stage_d.as<uint8_t>();
    FK_HIP(ctx, hipMemcpyAsync(d_pr, proofs, pr_b, hipMemcpyHostToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(d_w, w, w_b, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((count + 63) / 64), block(64);
    hipLaunchKernelGGL(agg_prepare_kernel, grid, block, 0, ctx->stream, (const uint8_t *)d_pr, (const uint64_t *)d_w, count, d_wa, d_b, d_wc, d_flag);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "agg_prepare_kernel");
    hipLaunchKernelGGL(agg_miller_kernel, grid, block, 0, ctx->stream, (const Affine<FqC> *)d_wa, (const Affine<Fq2C> *)d_b, count, d_f);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "agg_miller_kernel");
    size_t off = 0;
    for (uint32_t n = count; n > 1; n = (n + 1) / 2) {       // level widths count, ceil(count / 2), ..., 1 laid end to end: `lev` elements
        const uint32_t n_out = (n + 1) / 2;
        hipLaunchKernelGGL(f12_level_kernel, dim3((n_out + 63) / 64), block, 0, ctx->stream, (const F12C *)(d_f + off), n, d_f + off + n);
        hipLaunchKernelGGL(g1_level_kernel, dim3((n_out + 63) / 64), block, 0, ctx->stream, (const G1C *)(d_wc + off), n, d_wc + off + n);
        off += n;
    }
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "f12_level_kernel / g1_level_kernel");
    static_assert(sizeof(F12C) == sizeof(Fq12T<Fq>) && sizeof(G1C) == sizeof(Xyzz<Fq>), "the cold field type is layout-identical");
    FK_HIP(ctx, hipMemcpyAsync(o.flag.data(), d_flag, count, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(&o.f, d_f + off, sizeof o.f, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(&o.s_c, d_wc + off, sizeof o.s_c, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}

static int aggregate(fk_ctx *ctx, bool on_device, const uint8_t *vk, size_t vk_len, const uint64_t *inputs, uint32_t n_inputs, const uint8_t *proofs, uint32_t count,
                     const uint64_t *weights, uint8_t *wellformed, int *accept, fk_verify_agg_report *report) {
    if (!accept || (count && (!proofs || (n_inputs && !inputs)))) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "verify_aggregate: null argument");
    *accept = 0;
    fk_verify_agg_report rep;
    memset(&rep, 0, sizeof rep);
    rep.count = count; rep.equation_ok = 1;
    if (!count) { *accept = 1; if (report) *report = rep; return FK_OK; }
    uint32_t n_ic = 0;
    FK_TRY(vk_check(ctx, vk, vk_len, n_inputs, &n_ic));
    std::vector<uint64_t> drawn;
    if (weights) {
        for (uint32_t i = 0; i < count; i++)
            if (!(weights[2 * (size_t)i] | weights[2 * (size_t)i + 1]))
                FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "verify_aggregate: the weight of proof %u is zero -- it would drop the proof from the equation", i);
    } else {
        FK_TRY(draw_weights(ctx, count, drawn));
        weights = drawn.data();
    }
    bool vk_ok = true;
    const Affine<Fq> alpha = g1_from_borsh<Fq>(vk, &vk_ok);
    const Affine<Fq2> beta = g2_from_borsh<Fq>(vk + 64, &vk_ok), gamma = g2_from_borsh<Fq>(vk + 192, &vk_ok), delta = g2_from_borsh<Fq>(vk + 320, &vk_ok);
    std::vector<Affine<Fq>> ic(n_ic);
    for (uint32_t j = 0; j < n_ic; j++) ic[j] = g1_from_borsh<Fq>(vk + 452 + 64 * (size_t)j, &vk_ok);

    AggFront fr;
    fr.flag.assign(count, 0);
    // a key with a coordinate >= q: verify_one refuses every proof under it, so no proof is well-formed and nothing needs computing
    if (vk_ok) FK_TRY(on_device ? front_dev(ctx, proofs, count, weights, fr) : front_host(proofs, count, weights, fr));

    // ---- the tail: the sums in Fr, S_acc, the three fixed-G2 Miller loops, one final exponentiation
    Fr sum_w = Fr::zero();
    std::vector<Fr> u(n_inputs, Fr::zero());        // u_j = sum_i w_i x_ij
    for (uint32_t i = 0; i < count; i++) {
        if (!fr.flag[i]) continue;
        rep.n_wellformed++;
        Fr w = Fr::zero();
        w.v[0] = (uint32_t)weights[2 * (size_t)i]; w.v[1] = (uint32_t)(weights[2 * (size_t)i] >> 32);
        w.v[2] = (uint32_t)weights[2 * (size_t)i + 1]; w.v[3] = (uint32_t)(weights[2 * (size_t)i + 1] >> 32);
        w = Fr::to_mont(w);
        sum_w = Fr::add(sum_w, w);
        const Fr *x = (const Fr *)inputs + (size_t)i * n_inputs;
        for (uint32_t j = 0; j < n_inputs; j++) u[j] = Fr::add(u[j], Fr::mul(w, x[j]));
    }
    if (wellformed) memcpy(wellformed, fr.flag.data(), count);
    Affine<Fq> s_acc = Affine<Fq>::inf(), s_c = Affine<Fq>::inf();
    if (rep.n_wellformed) {
        auto negp = [](const Affine<Fq> &p) { return p.is_inf() ? p : Affine<Fq>{p.x, Fq::neg(p.y)}; };
        auto times = [](const Affine<Fq> &p, const Fr &k) { return Xyzz<Fq>::mul_scalar(Xyzz<Fq>::from_affine(p), Fr::from_mont(k).v); };
        Xyzz<Fq> acc = times(ic[0], sum_w);
        for (uint32_t j = 0; j < n_inputs; j++) acc.add(times(ic[j + 1], u[j]));
        s_acc = acc.to_affine();
        s_c = fr.s_c.to_affine();
        using F12 = Fq12T<Fq>;
        F12 m = F12::mul(fr.f, agg_miller<Fq>(negp(times(alpha, sum_w).to_affine()), beta));
        m = F12::mul(m, agg_miller<Fq>(negp(s_acc), gamma));
        m = F12::mul(m, agg_miller<Fq>(negp(s_c), delta));
        rep.equation_ok = final_exponentiation<Fq>(m).is_one() ? 1 : 0;
    }
    for (int k = 0; k < 4; k++) rep.sum_w[k] = (uint64_t)sum_w.v[2 * k] | (uint64_t)sum_w.v[2 * k + 1] << 32;
    static_assert(sizeof(Affine<Fq>) == 64, "raw affine G1");
    memcpy(rep.s_acc, &s_acc, 64); memcpy(rep.s_c, &s_c, 64);
    *accept = rep.equation_ok && rep.n_wellformed == count;
    if (report) *report = rep;
    if (rep.n_wellformed != count) {
        uint32_t first_bad = 0;
        while (fr.flag[first_bad]) first_bad++;
        char buf[200];
        snprintf(buf, sizeof buf, "note: %u of %u proofs are not well-formed (first: proof %u)%s -- left out of the equation, batch not accepted", count - rep.n_wellformed,
                 count, first_bad, vk_ok ? "" : ": the verifying key holds a coordinate that is not a canonical field element");
        ctx->err = buf;
    }
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_verify_aggregate(fk_ctx *ctx, const uint8_t *vk, size_t vk_len, const uint64_t *inputs, uint32_t n_inputs, const uint8_t *proofs, uint32_t count,
                        const uint64_t *weights, uint8_t *wellformed, int *accept, fk_verify_agg_report *report) {
    fk_ctx local;                  // host-only routine: usable without a GPU context; its message then goes to fk_last_error(NULL)
    if (!ctx) ctx = &local;
    const int rc = fk_guard(ctx, [&]() -> int { return aggregate(ctx, false, vk, vk_len, inputs, n_inputs, proofs, count, weights, wellformed, accept, report); });
    if (ctx == &local) { try { tls_error() = local.err; } catch (...) {} }
    return rc;
}

int fk_verify_aggregate_dev(fk_ctx *ctx, const uint8_t *vk, size_t vk_len, const uint64_t *inputs, uint32_t n_inputs, const uint8_t *proofs, uint32_t count,
                            const uint64_t *weights, uint8_t *wellformed, int *accept, fk_verify_agg_report *report) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    return aggregate(ctx, true, vk, vk_len, inputs, n_inputs, proofs, count, weights, wellformed, accept, report);
}); }

}  // extern "C"
