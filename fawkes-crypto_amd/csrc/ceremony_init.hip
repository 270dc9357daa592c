// Key ceremony, the start of phase 2 (include/fawkes_hip_ceremony_init.h): the initial proving key from a powers-of-tau
// transcript, and the transcript's check.
//
// Transforms over group elements: a work array of Xyzz points; pt_ntt_load_kernel applies the bit reversal, pt_ntt_stage_kernel is one
// radix-2 stage with one butterfly (u, v) -> (u + [w]v, u - [w]v) per lane, pt_affine_kernel brings everything back to affine with one
// Fermat inversion per lane.  The inverse's 1/n rides in the LAST stage (both operands of its butterflies are multiplied): half a
// multiplication per point more, where a pass of its own would cost one per point and the combination below would pay one per ONE term.
// The combination: per variable a sum of coeff * base[row] along its column of the CSC form, one task (a column, or a CI_SEG-term
// segment of a long one) per lane in ci_combine_kernel, the segments' partial sums folded by ci_fold_kernel level by level.
// The check: the existing weights and multi-scalar multiplication over an array and the same array one element on; pairings on the host.
// The host entries are plain loops over the generic double-and-add and the references the device is compared with.
#include "ceremony_shared.hpp"
#include "ntt_domain.hpp"
#include "../../include/fawkes_hip_ceremony.h"        // fk_ceremony_weights, fk_ceremony_weights_dev
#include "../../include/fawkes_hip_ceremony_init.h"
#include <string.h>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>

namespace fk {

// ------------------------------------------------------------------------------------------ a point times the lane's own scalar
// (K256, k256_of_mont, k256_shl and mul_affine_k256 live in ceremony_shared.hpp: powers.hip multiplies by a lane's own scalar too)
// k * p, p in XYZZ form (a butterfly's operand): complete additions
template <class F>
static FK_HD Xyzz<F> mul_xyzz_k256(const Xyzz<F> &p, K256 k) {
    Xyzz<F> acc = Xyzz<F>::inf();
#pragma nounroll
    for (int i = 0; i < 256; i++) {
        acc = Xyzz<F>::dbl(acc);
        if (k.w[3] >> 63) acc.add(p);
        k256_shl(k);
    }
    return acc;
}
static FK_HD uint64_t bit_reverse(uint64_t i, uint32_t bits) {
    uint64_t r = 0;
    for (uint32_t b = 0; b < bits; b++) { r = r << 1 | (i & 1); i >>= 1; }
    return r;
}

// ------------------------------------------------------------------------------------------ transforms over group elements (device)
template <class F>
__global__ __launch_bounds__(256) void pt_ntt_load_kernel(const Affine<F> *in, uint32_t log_n, Xyzz<F> *work) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_n) return;
    work[bit_reverse(i, log_n)] = Xyzz<F>::from_affine(in[i]);
}

// Stage s of log_n: lane t holds the butterfly of elements i0 = (t >> s) 2^(s+1) + j and i0 + 2^s, j = t mod 2^s, with the twiddle
// omega^(j 2^(log_n - 1 - s)) = tw_lo[e mod 2^L] * tw_hi[e >> L] of the domain's tables.  Twiddle index 0 multiplies nothing.
// SCALE (the inverse's last stage): u and the twiddle are multiplied by minv = 1/n as well.
// v is multiplied before u is loaded: the loop then holds two points and the scalar, not three.
template <class F, bool SCALE>
__global__ __launch_bounds__(64) void pt_ntt_stage_kernel(Xyzz<F> *work, uint32_t log_n, uint32_t s, const Fr *__restrict__ tw_lo, const Fr *__restrict__ tw_hi,
                                                          uint32_t L, Fr minv) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >> (log_n - 1)) return;
    const uint64_t j = t & (((uint64_t)1 << s) - 1);
    const uint64_t i0 = ((t >> s) << (s + 1)) + j, i1 = i0 + ((uint64_t)1 << s);
    const uint64_t e = j << (log_n - 1 - s);
    Xyzz<F> v = work[i1];
    if (SCALE || e) {
        Fr k = SCALE ? minv : Fr::one();
        if (e) {
            const Fr tw = Fr::mul(tw_lo[e & (((uint64_t)1 << L) - 1)], tw_hi[e >> L]);
            k = SCALE ? Fr::mul(tw, minv) : tw;
        }
        v = mul_xyzz_k256<F>(v, k256_of_mont(k));
    }
    Xyzz<F> u = work[i0];
    if (SCALE) u = mul_xyzz_k256<F>(u, k256_of_mont(minv));
    Xyzz<F> d = u;
    u.add(v);
    v.y = F::neg(v.y);
    d.add(v);
    work[i0] = u;
    work[i1] = d;
}

template <class F>
__global__ __launch_bounds__(64) void pt_affine_kernel(const Xyzz<F> *work, uint64_t n, Affine<F> *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = work[i].to_affine();
}

template <class F>
static int pt_affine_queue(fk_ctx *ctx, const Xyzz<F> *d_work, uint64_t n, Affine<F> *d_out) {
    if (!n) return FK_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_affine_kernel<F>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_work, n, d_out);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "pt_affine_kernel");
    return FK_OK;
}

static constexpr uint32_t PT_NTT_MAX_LOG = FK_FR_S - 1;

// d_pts: 2^log_n affine points, transformed in place through the context's work array
template <class F>
static int pt_ntt_queue(fk_ctx *ctx, Affine<F> *d_pts, uint32_t log_n, bool inverse) {
    if (log_n > PT_NTT_MAX_LOG) FK_SET_ERR(ctx, FK_ERR_DOMAIN_TOO_LARGE, "point transform: 2^%u points (max 2^%u)", log_n, PT_NTT_MAX_LOG);
    if (log_n == 0) return FK_OK;                      // one point: the transform is the identity, and 1/n = 1
    const uint64_t n = (uint64_t)1 << log_n;
    NttDomain *dm = nullptr;
    FK_TRY(get_domain(ctx, log_n, &dm));
    FK_HIP(ctx, ctx->ceremony_init.reserve(n * sizeof(Xyzz<F>)));
    Xyzz<F> *work = ctx->ceremony_init.as<Xyzz<F>>();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_ntt_load_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_pts, log_n, work);
    const int dir = inverse ? 1 : 0;
    const dim3 grid((unsigned)((n / 2 + 63) / 64));
    for (uint32_t s = 0; s < log_n; s++) {
        if (inverse && s == log_n - 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_ntt_stage_kernel<F, true>), grid, dim3(64), 0, ctx->stream, work, log_n, s, dm->tw_lo[dir], dm->tw_hi[dir], dm->L, dm->minv);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_ntt_stage_kernel<F, false>), grid, dim3(64), 0, ctx->stream, work, log_n, s, dm->tw_lo[dir], dm->tw_hi[dir], dm->L, dm->minv);
    }
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "pt_ntt_stage_kernel");
    return pt_affine_queue<F>(ctx, work, n, d_pts);
}

// ------------------------------------------------------------------------------------------ transforms over group elements (host reference)
// body(i) for i < n, the range cut into one piece per host thread (the references are plain loops; this only spreads them over the cores)
template <class Body>
static void host_par_for(uint64_t n, Body &&body) {
    const uint64_t nt = std::min<uint64_t>(std::max<unsigned>(host_threads(), 1u), n);
    if (nt <= 1) { for (uint64_t i = 0; i < n; i++) body(i); return; }
    std::vector<std::thread> th;
    for (uint64_t t = 0; t < nt; t++) th.emplace_back([&, t]() { for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; i++) body(i); });
    for (auto &x : th) x.join();
}

static Fr omega_for(uint32_t log_n) {
    const uint32_t root_w[8] = FK_FR_ROOT;
    Fr om;
    for (int i = 0; i < 8; i++) om.v[i] = root_w[i];
    for (uint32_t i = log_n; i < FK_FR_S; i++) om = Fr::sqr(om);
    return om;
}

template <class F>
static Xyzz<F> host_mul_xyzz(const Xyzz<F> &p, const Fr &k_mont) {
    const Fr k = Fr::from_mont(k_mont);
    return Xyzz<F>::mul_scalar(p, k.v);
}

// natural order in and out; the inverse multiplies every output by 1/n at the end
template <class F>
static void host_pt_ntt(std::vector<Affine<F>> &pts, uint32_t log_n, bool inverse) {
    const uint64_t n = (uint64_t)1 << log_n;
    std::vector<Xyzz<F>> a(n);
    for (uint64_t i = 0; i < n; i++) a[bit_reverse(i, log_n)] = Xyzz<F>::from_affine(pts[i]);
    Fr om = omega_for(log_n);
    if (inverse) om = Fr::inv(om);
    for (uint32_t s = 0; s < log_n; s++) {
        Fr wlen = om;                                                   // the 2^(s+1)-th root
        for (uint32_t i = s + 1; i < log_n; i++) wlen = Fr::sqr(wlen);
        const uint64_t half = (uint64_t)1 << s;
        std::vector<Fr> w(half);                                        // w[j] = wlen^j
        w[0] = Fr::one();
        for (uint64_t j = 1; j < half; j++) w[j] = Fr::mul(w[j - 1], wlen);
        host_par_for(n / 2, [&](uint64_t t) {
            const uint64_t j = t & (half - 1), i0 = ((t >> s) << (s + 1)) + j, i1 = i0 + half;
            const Xyzz<F> u = a[i0];
            Xyzz<F> v = j ? host_mul_xyzz<F>(a[i1], w[j]) : a[i1];
            Xyzz<F> sum = u, dif = u;
            sum.add(v);
            v.y = F::neg(v.y);
            dif.add(v);
            a[i0] = sum; a[i1] = dif;
        });
    }
    const Fr ninv = Fr::inv(Fr::from_u64(n));
    host_par_for(n, [&](uint64_t i) { pts[i] = (inverse && log_n ? host_mul_xyzz<F>(a[i], ninv) : a[i]).to_affine(); });
}

template <class F>
static int pt_ntt_host_entry(fk_ctx *c, const uint8_t *points, uint32_t log_n, int inverse, uint8_t *out) {
    if (!points || !out) FK_SET_ERR(c, FK_ERR_BAD_ARG, "point transform: null argument");
    if (log_n > PT_NTT_MAX_LOG) FK_SET_ERR(c, FK_ERR_DOMAIN_TOO_LARGE, "point transform: 2^%u points (max 2^%u)", log_n, PT_NTT_MAX_LOG);
    std::vector<Affine<F>> pts((size_t)1 << log_n);
    memcpy(pts.data(), points, pts.size() * sizeof(Affine<F>));
    host_pt_ntt<F>(pts, log_n, inverse != 0);
    memcpy(out, pts.data(), pts.size() * sizeof(Affine<F>));
    return FK_OK;
}

template <class F>
static int pt_ntt_staged_entry(fk_ctx *ctx, const uint8_t *points, uint32_t log_n, int inverse, uint8_t *out) {
    if (!points || !out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "point transform: null argument");
    if (log_n > PT_NTT_MAX_LOG) FK_SET_ERR(ctx, FK_ERR_DOMAIN_TOO_LARGE, "point transform: 2^%u points (max 2^%u)", log_n, PT_NTT_MAX_LOG);
    FK_TRY(scratch_claim(ctx, "point transform"));
    const size_t bytes = sizeof(Affine<F>) << log_n;
    HostStage st{ctx};
    Affine<F> *d = nullptr;
    FK_TRY(st.in(ctx->stage_a, points, bytes, &d));
    FK_TRY(pt_ntt_queue<F>(ctx, d, log_n, inverse != 0));
    return st.out(out, d, bytes);
}

template <class F>
static int pt_ntt_dev_entry(fk_ctx *ctx, void *d_points, uint32_t log_n, int inverse) {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!d_points) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "point transform: null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return pt_ntt_queue<F>(ctx, (Affine<F> *)d_points, log_n, inverse != 0);
}

// ------------------------------------------------------------------------------------------ the transcript and the circuit (host)
struct Powers {
    uint64_t m = 0;
    const G1Affine *tau_g1 = nullptr, *alpha_g1 = nullptr, *beta_g1 = nullptr;
    const G2Affine *tau_g2 = nullptr;
    G2Affine beta_g2;
};

// the prefixes a domain of m uses: 2m - 1 of tau_g1, m of the others
static int powers_arg(fk_ctx *ctx, const fk_powers_desc *p, uint64_t m, const char *who, Powers *out) {
    if (!p) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null transcript", who);
    if (!p->tau_g1 || !p->tau_g2 || !p->alpha_tau_g1 || !p->beta_tau_g1 || !p->beta_g2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the transcript lacks an array", who);
    if (((uintptr_t)p->tau_g1 | (uintptr_t)p->tau_g2 | (uintptr_t)p->alpha_tau_g1 | (uintptr_t)p->beta_tau_g1) & 15) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the transcript's arrays must be 16-byte aligned", who);
    const struct { const char *name; uint64_t have, need; } arr[4] ={{"tau_g1", p->n_tau_g1, 2 * m - 1}, {"tau_g2", p->n_tau_g2, m}, {"alpha_tau_g1", p->n_alpha_g1, m}, {"beta_tau_g1", p->n_beta_g1, m}};
    for (const auto &a : arr)
        if (a.have < a.need) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the transcript is too short: %s holds %llu elements, a domain of %llu needs %llu", who, a.name,
                                        (unsigned long long)a.have, (unsigned long long)m, (unsigned long long)a.need);
    static_assert(sizeof(G1Affine) == 64 && sizeof(G2Affine) == 128, "raw affine points");
    out->m = m;
    out->tau_g1 = (const G1Affine *)p->tau_g1; out->alpha_g1 = (const G1Affine *)p->alpha_tau_g1; out->beta_g1 = (const G1Affine *)p->beta_tau_g1;
    out->tau_g2 = (const G2Affine *)p->tau_g2;
    memcpy(&out->beta_g2, p->beta_g2, 128);
    return FK_OK;
}

// One set of columns: column v holds the terms [ptr[v], ptr[v + 1]) as (row, coefficient slot).
struct Columns { std::vector<uint64_t> ptr; std::vector<uint32_t> row, cidx; };
// The circuit by columns.  at, bt: the columns of A (with the term (1, num_gates + i) of input i) and B over a base of m rows; et: per
// variable its terms of A, B and C over the base [LG1 | LB | LA] of 3m rows: A's rows + m, B's rows + 2m, C's rows as they are.
// Coefficient slot 0 is ONE, slot 1 is r - 1, the others index `table` (Montgomery).
static constexpr uint32_t CI_ONE = 0, CI_MINUS_ONE = 1;
struct CircuitColumns {
    uint64_t m = 0, nv = 0, num_gates = 0;
    uint32_t log_m = 0, num_input = 0, num_aux = 0;
    Columns at, bt, et;
    std::vector<Fr> table;
};

static int circuit_columns(fk_ctx *ctx, const fk_r1cs *cs, const char *who, CircuitColumns *out) {
    if (!cs) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null constraint system", who);
    if (cs->num_input == 0) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: num_input must include the constant ONE", who);
    const uint64_t nv = (uint64_t)cs->num_input + cs->num_aux, rows = (uint64_t)cs->num_gates + cs->num_input;
    if (nv > 0xffffffffull || rows > 0xffffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the system is out of range", who);
    const uint32_t log_m = ceil_log2_u64(rows);
    if (log_m >= FK_FR_S) FK_SET_ERR(ctx, FK_ERR_DOMAIN_TOO_LARGE, "%s: evaluation domain 2^%u too large (max 2^%d)", who, log_m, FK_FR_S - 1);
    const uint64_t m = (uint64_t)1 << log_m;
    const uint64_t *ptrs[3] = {cs->a_ptr, cs->b_ptr, cs->c_ptr};
    const uint32_t *cols[3] = {cs->a_col, cs->b_col, cs->c_col};
    const uint64_t *vals[3] = {cs->a_val, cs->b_val, cs->c_val};
    for (int k = 0; k < 3; k++) {
        if (!ptrs[k]) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null row pointer", who);
        const uint64_t nnz = ptrs[k][cs->num_gates];
        if (nnz && !cols[k]) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null column array", who);
        for (uint64_t i = 0; i < nnz; i++) if (cols[k][i] >= nv) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: variable index %u out of range", who, cols[k][i]);
    }
    out->m = m; out->nv = nv; out->num_gates = cs->num_gates; out->log_m = log_m; out->num_input = cs->num_input; out->num_aux = cs->num_aux;
    const Fr one = Fr::one(), minus_one = Fr::neg(Fr::one());
    std::unordered_map<std::string, uint32_t> dict;
    out->table = {one, minus_one};
    dict.emplace(std::string((const char *)&one, 32), CI_ONE); dict.emplace(std::string((const char *)&minus_one, 32), CI_MINUS_ONE);
    // the three matrices by columns, gate order within a column
    Columns mt[3];
    for (int k = 0; k < 3; k++) {
        const uint64_t nnz = ptrs[k][cs->num_gates], extra = k == 0 ? cs->num_input : 0;
        Columns &c = mt[k];
        c.ptr.assign(nv + 1, 0);
        for (uint64_t i = 0; i < nnz; i++) c.ptr[cols[k][i] + 1]++;
        for (uint64_t v = 0; v < extra; v++) c.ptr[v + 1]++;
        for (uint64_t v = 0; v < nv; v++) c.ptr[v + 1] += c.ptr[v];
        c.row.resize(nnz + extra); c.cidx.resize(nnz + extra);
        std::vector<uint64_t> cur(c.ptr.begin(), c.ptr.end() - 1);
        for (uint64_t g = 0; g < cs->num_gates; g++)
            for (uint64_t i = ptrs[k][g]; i < ptrs[k][g + 1]; i++) {
                uint32_t ci = CI_ONE;
                if (vals[k]) {
                    const std::string key((const char *)(vals[k] + 4 * i), 32);
                    auto it = dict.find(key);
                    if (it == dict.end()) { Fr v; memcpy(&v, vals[k] + 4 * i, 32); it = dict.emplace(key, (uint32_t)out->table.size()).first; out->table.push_back(v); }
                    ci = it->second;
                }
                const uint64_t pos = cur[cols[k][i]]++;
                c.row[pos] = (uint32_t)g; c.cidx[pos] = ci;
            }
        for (uint64_t v = 0; v < extra; v++) { const uint64_t pos = cur[v]++; c.row[pos] = (uint32_t)(cs->num_gates + v); c.cidx[pos] = CI_ONE; }
    }
    Columns &e = out->et;
    e.ptr.assign(nv + 1, 0);
    for (uint64_t v = 0; v < nv; v++) {
        e.ptr[v + 1] = e.ptr[v];
        for (int k = 0; k < 3; k++) e.ptr[v + 1] += mt[k].ptr[v + 1] - mt[k].ptr[v];
    }
    e.row.resize(e.ptr[nv]); e.cidx.resize(e.ptr[nv]);
    const uint64_t shift[3] = {m, 2 * m, 0};
    for (uint64_t v = 0; v < nv; v++) {
        uint64_t pos = e.ptr[v];
        for (int k = 0; k < 3; k++)
            for (uint64_t i = mt[k].ptr[v]; i < mt[k].ptr[v + 1]; i++, pos++) { e.row[pos] = (uint32_t)(mt[k].row[i] + shift[k]); e.cidx[pos] = mt[k].cidx[i]; }
    }
    out->at = std::move(mt[0]); out->bt = std::move(mt[1]);
    return FK_OK;
}

static void vk_write(const Powers &pw, uint8_t vk_out[6 * 128]) {
    const G1Affine g1 = g1_gen();
    const G2Affine g2 = g2_gen();
    memset(vk_out, 0, 6 * 128);
    memcpy(vk_out + 0 * 128, &pw.alpha_g1[0], 64); memcpy(vk_out + 1 * 128, &pw.beta_g1[0], 64); memcpy(vk_out + 2 * 128, &pw.beta_g2, 128);
    memcpy(vk_out + 3 * 128, &g2, 128); memcpy(vk_out + 4 * 128, &g1, 64); memcpy(vk_out + 5 * 128, &g2, 128);
}

// ------------------------------------------------------------------------------------------ the initial key (host reference)
template <class F>
static Affine<F> host_column_sum(const Columns &c, uint64_t v, const std::vector<Fr> &table, const std::vector<Affine<F>> &base) {
    Xyzz<F> acc = Xyzz<F>::inf();
    for (uint64_t k = c.ptr[v]; k < c.ptr[v + 1]; k++) {
        const Xyzz<F> b = Xyzz<F>::from_affine(base[c.row[k]]);
        acc.add(c.cidx[k] == CI_ONE ? b : host_mul_xyzz<F>(b, table[c.cidx[k]]));
    }
    return acc.to_affine();
}

static int key_from_powers_host(fk_ctx *c, const fk_powers_desc *p, const fk_r1cs *cs, uint8_t *h_out, uint8_t *l_out, uint8_t *a_out, uint8_t *b_g1_out,
                                uint8_t *b_g2_out, uint64_t counts_out[2], uint8_t vk_out[6 * 128], uint8_t *ic_out) {
    const char *who = "key from powers (host)";
    CircuitColumns cc;
    FK_TRY(circuit_columns(c, cs, who, &cc));
    if (!counts_out || !vk_out || !ic_out) FK_SET_ERR(c, FK_ERR_BAD_ARG, "%s: null output", who);
    Powers pw;
    FK_TRY(powers_arg(c, p, cc.m, who, &pw));
    const uint64_t m = cc.m, nv = cc.nv;
    if ((m > 1 && !h_out) || (cc.num_aux && !l_out) || !a_out || !b_g1_out || !b_g2_out) FK_SET_ERR(c, FK_ERR_BAD_ARG, "%s: null output", who);
    std::vector<G1Affine> lag(3 * m);                    // [LG1 | LB | LA]
    std::vector<G2Affine> lg2(pw.tau_g2, pw.tau_g2 + m);
    const G1Affine *src[3] = {pw.tau_g1, pw.beta_g1, pw.alpha_g1};
    for (int k = 0; k < 3; k++) {
        std::vector<G1Affine> t(src[k], src[k] + m);
        host_pt_ntt<Fq>(t, cc.log_m, true);
        std::copy(t.begin(), t.end(), lag.begin() + k * m);
    }
    host_pt_ntt<Fq2>(lg2, cc.log_m, true);
    for (uint64_t i = 0; i + 1 < m; i++) {
        G1Xyzz acc = G1Xyzz::from_affine(pw.tau_g1[i + m]);
        acc.add(G1Xyzz::from_affine(affine_neg_if(pw.tau_g1[i], true)));
        const G1Affine h = acc.to_affine();
        memcpy(h_out + 64 * i, &h, 64);
    }
    std::vector<G1Affine> a_all(nv), b1_all(nv), e_all(nv);
    std::vector<G2Affine> b2_all(nv);
    host_par_for(nv, [&](uint64_t v) {
        a_all[v] = host_column_sum<Fq>(cc.at, v, cc.table, lag); b1_all[v] = host_column_sum<Fq>(cc.bt, v, cc.table, lag);
        e_all[v] = host_column_sum<Fq>(cc.et, v, cc.table, lag); b2_all[v] = host_column_sum<Fq2>(cc.bt, v, cc.table, lg2);
    });
    uint64_t n_a = 0, n_b = 0;
    for (uint64_t v = 0; v < nv; v++) {
        const G1Affine &a = a_all[v], &b1 = b1_all[v], &e = e_all[v];
        const G2Affine &b2 = b2_all[v];
        if (!a.is_inf()) memcpy(a_out + 64 * n_a++, &a, 64);
        if (!b1.is_inf()) { memcpy(b_g1_out + 64 * n_b, &b1, 64); memcpy(b_g2_out + 128 * n_b, &b2, 128); n_b++; }
        if (v < cc.num_input) memcpy(ic_out + 64 * v, &e, 64); else memcpy(l_out + 64 * (v - cc.num_input), &e, 64);
    }
    counts_out[0] = n_a; counts_out[1] = n_b;
    vk_write(pw, vk_out);
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ the initial key (device)
// h[i] = tau[i + m] - tau[i], i < m - 1
__global__ __launch_bounds__(64) void ci_h_kernel(const G1Affine *__restrict__ tau, uint64_t m, G1Affine *__restrict__ h) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= m) return;
    G1Xyzz acc = G1Xyzz::from_affine(tau[i + m]);
    acc.add_mixed(affine_neg_if(tau[i], true));
    h[i] = acc.to_affine();
}

// Columns longer than CI_SEG terms are cut into segments of CI_SEG, one lane each; their partial sums are folded CI_SEG at a time, level
// by level, until one sum per column is left (the column of ONE in a real circuit has millions of terms).
static constexpr uint64_t CI_SEG = 16;
struct CombTask { uint64_t lo, hi, out; };      // combine: terms [lo, hi) of the columns; fold: elements [lo, hi) of the work array -> work[out]
struct CombPlan {
    std::vector<CombTask> tasks;                 // one per light column (out = the variable) and per segment (out = a partial sum behind the nv sums)
    std::vector<std::vector<CombTask>> folds;    // level by level; a task reads what earlier launches wrote
    uint64_t work = 0;                           // elements of the work array: nv sums and every partial sum
};
static CombPlan comb_plan(const Columns &c, uint64_t nv) {
    CombPlan pl;
    uint64_t next = nv;
    for (uint64_t v = 0; v < nv; v++) {
        const uint64_t lo = c.ptr[v], hi = c.ptr[v + 1];
        if (hi - lo <= CI_SEG) { pl.tasks.push_back(CombTask{lo, hi, v}); continue; }
        uint64_t first = next;
        for (uint64_t k = lo; k < hi; k += CI_SEG) pl.tasks.push_back(CombTask{k, k + CI_SEG < hi ? k + CI_SEG : hi, next++});
        size_t level = 0;
        while (next - first > CI_SEG) {
            if (pl.folds.size() <= level) pl.folds.emplace_back();
            const uint64_t end = next;
            for (uint64_t k = first; k < end; k += CI_SEG) pl.folds[level].push_back(CombTask{k, k + CI_SEG < end ? k + CI_SEG : end, next++});
            first = end; level++;
        }
        if (pl.folds.size() <= level) pl.folds.emplace_back();
        pl.folds[level].push_back(CombTask{first, next, v});
    }
    pl.work = next;
    return pl;
}

// work[task.out] = sum over the task's terms of coeff * base[row]: ONE is a mixed addition, r - 1 a mixed subtraction, everything else a
// multiplication by the lane's own coefficient.  A base point at infinity contributes nothing.
template <class F>
__global__ __launch_bounds__(64) void ci_combine_kernel(const CombTask *__restrict__ tasks, uint64_t n_tasks, const uint32_t *__restrict__ row, const uint32_t *__restrict__ cidx,
                                                        const Fr *__restrict__ table, const Affine<F> *__restrict__ base, Xyzz<F> *__restrict__ work) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tasks) return;
    const CombTask tk = tasks[t];
    Xyzz<F> acc = Xyzz<F>::inf();
    for (uint64_t k = tk.lo; k < tk.hi; k++) {
        const Affine<F> p = base[row[k]];
        const uint32_t ci = cidx[k];
        if (p.is_inf()) continue;
        if (ci <= CI_MINUS_ONE) acc.add_mixed_nz(affine_neg_if(p, ci == CI_MINUS_ONE));
        else acc.add(mul_affine_k256<F>(p, k256_of_mont(table[ci])));
    }
    work[tk.out] = acc;
}

template <class F>
__global__ __launch_bounds__(64) void ci_fold_kernel(const CombTask *__restrict__ tasks, uint64_t n_tasks, Xyzz<F> *work) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tasks) return;
    const CombTask tk = tasks[t];
    Xyzz<F> acc = Xyzz<F>::inf();
    for (uint64_t k = tk.lo; k < tk.hi; k++) acc.add(work[k]);
    work[tk.out] = acc;
}

template <class F>
__global__ __launch_bounds__(256) void ci_flag_kernel(const Affine<F> *__restrict__ pts, uint64_t n, uint8_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = pts[i].is_inf() ? 0 : 1;
}

template <class T>
__global__ __launch_bounds__(256) void ci_gather_kernel(const T *__restrict__ in, const uint32_t *__restrict__ idx, uint64_t n, T *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[idx[i]];
}

template <class T>
static int to_device(fk_ctx *ctx, DevArr<T> &d, const T *host, size_t n) {
    if (d.alloc(n ? n : 1) != hipSuccess) FK_SET_ERR(ctx, FK_ERR_OOM, "key from powers: device allocation failed");
    if (n) FK_HIP(ctx, hipMemcpyAsync(d.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return FK_OK;
}

// the columns `c` and their plan on the device
struct DevColumns {
    DevArr<uint32_t> row, cidx;
    DevArr<CombTask> tasks;
    std::vector<DevArr<CombTask>> folds;
    CombPlan plan;
};
static int columns_to_device(fk_ctx *ctx, const Columns &c, uint64_t nv, DevColumns *out) {
    out->plan = comb_plan(c, nv);
    FK_TRY(to_device(ctx, out->row, c.row.data(), c.row.size()));
    FK_TRY(to_device(ctx, out->cidx, c.cidx.data(), c.cidx.size()));
    FK_TRY(to_device(ctx, out->tasks, out->plan.tasks.data(), out->plan.tasks.size()));
    out->folds.resize(out->plan.folds.size());
    for (size_t i = 0; i < out->folds.size(); i++) FK_TRY(to_device(ctx, out->folds[i], out->plan.folds[i].data(), out->plan.folds[i].size()));
    return FK_OK;
}

// d_out[v] = sum over column v of coeff * d_base[row], affine, for the nv variables; the Xyzz sums live in the context's work array
template <class F>
static int combine_queue(fk_ctx *ctx, const DevColumns &c, uint64_t nv, const Fr *d_table, const Affine<F> *d_base, Affine<F> *d_out) {
    if (!nv) return FK_OK;
    FK_HIP(ctx, ctx->ceremony_init.reserve(c.plan.work * sizeof(Xyzz<F>)));
    Xyzz<F> *work = ctx->ceremony_init.as<Xyzz<F>>();
    const uint64_t nt = c.plan.tasks.size();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_combine_kernel<F>), dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, ctx->stream, c.tasks.p, nt, c.row.p, c.cidx.p, d_table, d_base, work);
    for (size_t i = 0; i < c.folds.size(); i++) {
        const uint64_t nf = c.plan.folds[i].size();
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_fold_kernel<F>), dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, ctx->stream, c.folds[i].p, nf, work);
    }
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "ci_combine_kernel");
    return pt_affine_queue<F>(ctx, work, nv, d_out);
}

static int key_from_powers_dev(fk_ctx *ctx, const fk_powers_desc *p, const fk_r1cs *cs, uint32_t flags, fk_key **out_key, uint8_t vk_out[6 * 128], uint8_t *ic_out) {
    const char *who = "key from powers";
    if (!out_key || !vk_out || !ic_out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    *out_key = nullptr;
    if (flags & ~(uint32_t)FK_KEY_NO_LEVELS) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: flags must be 0 or FK_KEY_NO_LEVELS", who);
    FK_TRY(lanes_claim(ctx, who));
    CircuitColumns cc;
    FK_TRY(circuit_columns(ctx, cs, who, &cc));
    Powers pw;
    FK_TRY(powers_arg(ctx, p, cc.m, who, &pw));
    const uint64_t m = cc.m, nv = cc.nv;
    hipStream_t st = ctx->stream;
    auto drop = [ctx](fk_key *k) { fk_key_free(ctx, k); };
    std::unique_ptr<fk_key, decltype(drop)> k(new fk_key(), drop);
    k->m = m; k->num_input = cc.num_input; k->num_aux = cc.num_aux; k->n_h = m - 1; k->n_l = cc.num_aux;
    struct WorkGuard { fk_ctx *c; ~WorkGuard() { c->ceremony_init.release(); } } work_guard{ctx};      // nothing stays allocated but the key
    {
        // ---- h, and the four Lagrange bases
        DevArr<G1Affine> d_tau, d_lag;
        DevArr<G2Affine> d_lg2;
        FK_TRY(to_device(ctx, d_tau, pw.tau_g1, (size_t)(2 * m - 1)));
        FK_HIP(ctx, hipMalloc((void **)&k->d_h, (k->n_h + 1) * sizeof(G1Affine)));       // (the arrays as fk_setup allocates them: one spare element each)
        if (m > 1) hipLaunchKernelGGL(ci_h_kernel, dim3((unsigned)((m - 1 + 63) / 64)), dim3(64), 0, st, d_tau.p, m, k->d_h);
        FK_HIP(ctx, hipGetLastError());
        if (d_lag.alloc(3 * m) != hipSuccess) FK_SET_ERR(ctx, FK_ERR_OOM, "%s: device allocation failed", who);
        FK_HIP(ctx, hipMemcpyAsync(d_lag.p, d_tau.p, m * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
        FK_HIP(ctx, hipMemcpyAsync(d_lag.p + m, pw.beta_g1, m * sizeof(G1Affine), hipMemcpyHostToDevice, st));
        FK_HIP(ctx, hipMemcpyAsync(d_lag.p + 2 * m, pw.alpha_g1, m * sizeof(G1Affine), hipMemcpyHostToDevice, st));
        FK_TRY(to_device(ctx, d_lg2, pw.tau_g2, (size_t)m));
        for (int i = 0; i < 3; i++) FK_TRY(pt_ntt_queue<Fq>(ctx, d_lag.p + i * m, cc.log_m, true));
        FK_TRY(pt_ntt_queue<Fq2>(ctx, d_lg2.p, cc.log_m, true));
        FK_HIP(ctx, hipStreamSynchronize(st));
        d_tau.reset();
        // ---- the sums per variable
        DevArr<Fr> d_table;
        FK_TRY(to_device(ctx, d_table, cc.table.data(), cc.table.size()));
        DevArr<G1Affine> d_a_all, d_b1_all, d_e;
        DevArr<G2Affine> d_b2_all;
        if (d_a_all.alloc(nv) != hipSuccess || d_b1_all.alloc(nv) != hipSuccess || d_e.alloc(nv) != hipSuccess || d_b2_all.alloc(nv) != hipSuccess)
            FK_SET_ERR(ctx, FK_ERR_OOM, "%s: device allocation failed", who);
        {
            DevColumns dc;
            FK_TRY(columns_to_device(ctx, cc.at, nv, &dc));
            FK_TRY(combine_queue<Fq>(ctx, dc, nv, d_table.p, d_lag.p, d_a_all.p));
            FK_HIP(ctx, hipStreamSynchronize(st));
        }
        {
            DevColumns dc;
            FK_TRY(columns_to_device(ctx, cc.bt, nv, &dc));
            FK_TRY(combine_queue<Fq>(ctx, dc, nv, d_table.p, d_lag.p, d_b1_all.p));
            FK_TRY(combine_queue<Fq2>(ctx, dc, nv, d_table.p, d_lg2.p, d_b2_all.p));
            FK_HIP(ctx, hipStreamSynchronize(st));
        }
        {
            DevColumns dc;
            FK_TRY(columns_to_device(ctx, cc.et, nv, &dc));
            FK_TRY(combine_queue<Fq>(ctx, dc, nv, d_table.p, d_lag.p, d_e.p));
            FK_HIP(ctx, hipStreamSynchronize(st));
        }
        // ---- a, b_g1, b_g2: the sums that are not the point at infinity, in variable order; the counts before the arrays
        DevArr<uint8_t> d_flag;
        if (d_flag.alloc(2 * nv) != hipSuccess) FK_SET_ERR(ctx, FK_ERR_OOM, "%s: device allocation failed", who);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_flag_kernel<Fq>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, d_a_all.p, nv, d_flag.p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_flag_kernel<Fq>), dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, d_b1_all.p, nv, d_flag.p + nv);
        FK_HIP(ctx, hipGetLastError());
        std::vector<uint8_t> flag(2 * nv);
        FK_HIP(ctx, hipMemcpyAsync(flag.data(), d_flag.p, 2 * nv, hipMemcpyDeviceToHost, st));
        FK_HIP(ctx, hipStreamSynchronize(st));
        std::vector<uint32_t> idx_a, idx_b;
        for (uint64_t v = 0; v < nv; v++) { if (flag[v]) idx_a.push_back((uint32_t)v); if (flag[nv + v]) idx_b.push_back((uint32_t)v); }
        k->n_a = idx_a.size(); k->n_b = idx_b.size();
        FK_TRY(key_plan_slices(ctx, k.get(), FK_Z_EQUAL_SPLIT, FK_Z_EQUAL_SPLIT));
        FK_HIP(ctx, hipMalloc((void **)&k->d_l, (k->n_l + 1) * sizeof(G1Affine)));
        FK_HIP(ctx, hipMalloc((void **)&k->d_a, (k->n_a + 1) * sizeof(G1Affine)));
        FK_HIP(ctx, hipMalloc((void **)&k->d_b1, (k->n_b + 1) * sizeof(G1Affine)));
        FK_HIP(ctx, hipMalloc((void **)&k->d_b2, (k->n_b + 1) * sizeof(G2Affine)));
        DevArr<uint32_t> d_ia, d_ib;
        FK_TRY(to_device(ctx, d_ia, idx_a.data(), idx_a.size()));
        FK_TRY(to_device(ctx, d_ib, idx_b.data(), idx_b.size()));
        if (k->n_a) hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_gather_kernel<G1Affine>), dim3((unsigned)((k->n_a + 255) / 256)), dim3(256), 0, st, d_a_all.p, d_ia.p, k->n_a, k->d_a);
        if (k->n_b) hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_gather_kernel<G1Affine>), dim3((unsigned)((k->n_b + 255) / 256)), dim3(256), 0, st, d_b1_all.p, d_ib.p, k->n_b, k->d_b1);
        if (k->n_b) hipLaunchKernelGGL(HIP_KERNEL_NAME(ci_gather_kernel<G2Affine>), dim3((unsigned)((k->n_b + 255) / 256)), dim3(256), 0, st, d_b2_all.p, d_ib.p, k->n_b, k->d_b2);
        FK_HIP(ctx, hipGetLastError());
        if (k->n_l) FK_HIP(ctx, hipMemcpyAsync(k->d_l, d_e.p + cc.num_input, k->n_l * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
        FK_HIP(ctx, hipMemcpyAsync(ic_out, d_e.p, (size_t)cc.num_input * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
        FK_HIP(ctx, hipStreamSynchronize(st));
    }      // every temporary goes before the fixed-base levels are sized against free memory
    ctx->ceremony_init.release();
    k->alpha_g1 = pw.alpha_g1[0]; k->beta_g1 = pw.beta_g1[0]; k->beta_g2 = pw.beta_g2;
    k->delta_g1 = g1_gen(); k->delta_g2 = g2_gen();
    vk_write(pw, vk_out);
    if (!(flags & FK_KEY_NO_LEVELS)) FK_TRY(key_precompute(ctx, k.get()));
    *out_key = k.release();
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ the transcript check
// the verdict from the transcript's single points and the eight sums: s1 = S, S' of tau_g1, alpha, beta; s2 = S, S' of tau_g2
static void powers_verdict(const Powers &pw, const G1Affine s1[6], const G2Affine s2[2], const uint8_t seed[32], fk_powers_report *rep) {
    const G1Affine g1 = g1_gen();
    const G2Affine g2 = g2_gen();
    memset(rep, 0, sizeof *rep);
    memcpy(rep->seed, seed, 32);
    rep->gen_ok = !memcmp(&pw.tau_g1[0], &g1, 64) && !memcmp(&pw.tau_g2[0], &g2, 128);
    rep->tau_pair = pairing_eq(pw.tau_g1[1], g2, g1, pw.tau_g2[1]);
    rep->ratio_tau_g1 = pairing_eq(s1[1], g2, s1[0], pw.tau_g2[1]);
    rep->ratio_alpha = pairing_eq(s1[3], g2, s1[2], pw.tau_g2[1]);
    rep->ratio_beta = pairing_eq(s1[5], g2, s1[4], pw.tau_g2[1]);
    rep->ratio_tau_g2 = pairing_eq(pw.tau_g1[1], s2[0], g1, s2[1]);
    rep->beta_pair = pairing_eq(pw.beta_g1[0], g2, g1, pw.beta_g2);
    memcpy(rep->s_tau_g1, &s1[0], 64); memcpy(rep->s_tau_g1_next, &s1[1], 64); memcpy(rep->s_alpha, &s1[2], 64); memcpy(rep->s_alpha_next, &s1[3], 64);
    memcpy(rep->s_beta, &s1[4], 64); memcpy(rep->s_beta_next, &s1[5], 64); memcpy(rep->s_tau_g2, &s2[0], 128); memcpy(rep->s_tau_g2_next, &s2[1], 128);
    rep->accept = rep->gen_ok && rep->tau_pair && rep->ratio_tau_g1 && rep->ratio_tau_g2 && rep->ratio_alpha && rep->ratio_beta && rep->beta_pair;
}

static int powers_check_arg(fk_ctx *ctx, const fk_powers_desc *p, uint64_t m, fk_powers_report *report, Powers *pw) {
    if (!report) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "powers check: null argument");
    if (m < 2 || m >= ((uint64_t)1 << FK_FR_S)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "powers check: m must be at least 2 and below 2^%d", FK_FR_S);
    return powers_arg(ctx, p, m, "powers check", pw);
}

template <class F>
static void host_weighted_sums(const Affine<F> *t, uint64_t n, const std::vector<Fr> &w, Affine<F> out[2]) {
    std::vector<Xyzz<F>> term(n ? 2 * (n - 1) : 0);
    host_par_for(n ? n - 1 : 0, [&](uint64_t i) {
        const K256 k = k256_of_mont(w[i]);
        term[2 * i] = Xyzz<F>::mul_affine_bits(t[i], k.w[0], k.w[1], 128);
        term[2 * i + 1] = Xyzz<F>::mul_affine_bits(t[i + 1], k.w[0], k.w[1], 128);
    });
    Xyzz<F> s = Xyzz<F>::inf(), s_next = Xyzz<F>::inf();
    for (uint64_t i = 0; i + 1 < n; i++) { s.add(term[2 * i]); s_next.add(term[2 * i + 1]); }
    out[0] = s.to_affine(); out[1] = s_next.to_affine();
}

static int powers_check_host(fk_ctx *c, const fk_powers_desc *p, uint64_t m, const uint8_t *seed, fk_powers_report *report) {
    if (!seed) FK_SET_ERR(c, FK_ERR_BAD_ARG, "powers check: null argument");
    Powers pw;
    FK_TRY(powers_check_arg(c, p, m, report, &pw));
    std::vector<Fr> w(2 * m - 2);
    if (fk_ceremony_weights(seed, w.size(), (uint64_t *)w.data()) != FK_OK) FK_SET_ERR(c, FK_ERR_BAD_ARG, "powers check: the weights could not be made");
    G1Affine s1[6];
    G2Affine s2[2];
    host_weighted_sums<Fq>(pw.tau_g1, 2 * m - 1, w, s1);
    host_weighted_sums<Fq>(pw.alpha_g1, m, w, s1 + 2);
    host_weighted_sums<Fq>(pw.beta_g1, m, w, s1 + 4);
    host_weighted_sums<Fq2>(pw.tau_g2, m, w, s2);
    powers_verdict(pw, s1, s2, seed, report);
    return FK_OK;
}

static int powers_check_dev(fk_ctx *ctx, const fk_powers_desc *p, uint64_t m, const uint8_t *seed_in, fk_powers_report *report) {
    Powers pw;
    FK_TRY(powers_check_arg(ctx, p, m, report, &pw));
    FK_TRY(lanes_claim(ctx, "powers check"));
    uint8_t seed[32];
    if (seed_in) memcpy(seed, seed_in, 32); else FK_TRY(draw_seed(ctx, seed, "powers check"));
    // the arrays in the staging buffers, the weights once for the longest array
    HostStage st{ctx};
    G1Affine *d_t1[3];
    G2Affine *d_t2 = nullptr;
    const G1Affine *src[3] = {pw.tau_g1, pw.alpha_g1, pw.beta_g1};
    const uint64_t len[3] = {2 * m - 1, m, m};
    DevBuf *buf[3] = {&ctx->stage_a, &ctx->stage_b, &ctx->stage_c};
    for (int i = 0; i < 3; i++) FK_TRY(st.in(*buf[i], src[i], len[i] * sizeof(G1Affine), &d_t1[i]));
    FK_TRY(st.in(ctx->stage_d, pw.tau_g2, m * sizeof(G2Affine), &d_t2));
    const size_t nw = (size_t)(2 * m - 2);
    FK_HIP(ctx, ctx->ceremony.reserve(nw * sizeof(Fr)));
    Fr *d_w = ctx->ceremony.as<Fr>();
    FK_TRY(fk_ceremony_weights_dev(ctx, seed, nw, d_w));
    G1Affine s1[6];
    G2Affine s2[2];
    for (int i = 0; i < 6; i++) {
        G1Xyzz r;
        FK_TRY(msm_g1_dev(ctx, d_t1[i / 2] + (i & 1), d_w, (size_t)(len[i / 2] - 1), &r));
        s1[i] = r.to_affine();
    }
    for (int i = 0; i < 2; i++) {
        G2Xyzz r;
        FK_TRY(msm_g2_dev(ctx, d_t2 + i, d_w, (size_t)(m - 1), &r));
        s2[i] = r.to_affine();
    }
    powers_verdict(pw, s1, s2, seed, report);
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_g1_ntt_dev(fk_ctx *ctx, void *d_points, uint32_t log_n, int inverse) { return fk_guard(ctx, [&]() -> int { return pt_ntt_dev_entry<Fq>(ctx, d_points, log_n, inverse); }); }
int fk_g2_ntt_dev(fk_ctx *ctx, void *d_points, uint32_t log_n, int inverse) { return fk_guard(ctx, [&]() -> int { return pt_ntt_dev_entry<Fq2>(ctx, d_points, log_n, inverse); }); }

int fk_g1_ntt(fk_ctx *ctx, const uint8_t *points, uint32_t log_n, int inverse, uint8_t *out) {
    if (!ctx) return host_entry([&](fk_ctx *c) -> int { return pt_ntt_host_entry<Fq>(c, points, log_n, inverse, out); });
    return fk_guard(ctx, [&]() -> int { return pt_ntt_staged_entry<Fq>(ctx, points, log_n, inverse, out); });
}
int fk_g2_ntt(fk_ctx *ctx, const uint8_t *points, uint32_t log_n, int inverse, uint8_t *out) {
    if (!ctx) return host_entry([&](fk_ctx *c) -> int { return pt_ntt_host_entry<Fq2>(c, points, log_n, inverse, out); });
    return fk_guard(ctx, [&]() -> int { return pt_ntt_staged_entry<Fq2>(ctx, points, log_n, inverse, out); });
}

int fk_key_from_powers(fk_ctx *ctx, const fk_powers_desc *p, const fk_r1cs *cs, uint32_t flags, fk_key **out_key, uint8_t vk_out[6 * 128], uint8_t *ic_out) {
    return fk_guard(ctx, [&]() -> int {
        FK_RANGE("fk_key_from_powers");
        if (!ctx) return FK_ERR_BAD_ARG;
        return key_from_powers_dev(ctx, p, cs, flags, out_key, vk_out, ic_out);
    });
}

int fk_key_from_powers_host(const fk_powers_desc *p, const fk_r1cs *cs, uint8_t *h_out, uint8_t *l_out, uint8_t *a_out, uint8_t *b_g1_out,
                            uint8_t *b_g2_out, uint64_t counts_out[2], uint8_t vk_out[6 * 128], uint8_t *ic_out) {
    return host_entry([&](fk_ctx *c) -> int { return key_from_powers_host(c, p, cs, h_out, l_out, a_out, b_g1_out, b_g2_out, counts_out, vk_out, ic_out); });
}

int fk_powers_check(fk_ctx *ctx, const fk_powers_desc *p, uint64_t m, const uint8_t *seed, fk_powers_report *report) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_powers_check");
    if (!ctx) return FK_ERR_BAD_ARG;
    return powers_check_dev(ctx, p, m, seed, report);
}); }

int fk_powers_check_host(const fk_powers_desc *p, uint64_t m, const uint8_t seed[32], fk_powers_report *report) {
    return host_entry([&](fk_ctx *c) -> int { return powers_check_host(c, p, m, seed, report); });
}

}  // extern "C"
