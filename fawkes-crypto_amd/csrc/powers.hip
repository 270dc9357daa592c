// Key ceremony, phase 1 (include/fawkes_hip_powers.h): contribute to a powers-of-tau transcript, validate the points of one,
// check an update.
//
// Contribute: powers_scale_kernel, one point per lane, every lane with its OWN scalar c x^(first + i) -- derived in the kernel (a power
// by squaring and one product, ~130 products against ~4.9 k of the multiplication), walked by shifting (K256, ceremony_shared.hpp).  The
// lanes' bits differ, so a wave executes the addition in practically every step: 256 doublings and 256 mixed additions per point, not the
// per-lane average.  Validate: points_validate_kernel, one point per lane, the subgroup test of G2 a multiplication by r whose
// non-adjacent form travels by value (mul_naf: the digits live in scalar registers, every branch on a digit is wave-uniform).  The update
// check stages and validates `after`, runs the existing transcript check on it and three more pairing equations on the host.
// The host entries are plain loops (powers_host.hpp) and the references the device is compared with.
#include "powers_host.hpp"
#include "poseidon.hpp"          // Seedbox::fr_below_modulus, fr_from_limbs
#include "../../include/fawkes_hip_powers.h"

namespace fk {

static_assert(sizeof(PointsCount) == sizeof(fk_points_report), "the device record is the report");
static_assert(sizeof(G1Affine) == 64 && sizeof(G2Affine) == 128, "raw affine points");

// ------------------------------------------------------------------------------------------ a point times its own power of x
// A lane whose input is the point at infinity runs the loop on the generator and stores infinity: it stays in step with its wave (the rule
// of g1_scale_kernel).  in == out is allowed (a lane reads its own element before it writes it), hence no __restrict__.
template <class F>
__global__ __launch_bounds__(64) void powers_scale_kernel(const Affine<F> *in, uint64_t n, uint64_t first, Fr x, Fr c, Affine<F> *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const K256 k = k256_of_mont(Fr::mul(Fr::pow_u64(x, first + i), c));
    Affine<F> p = in[i];
    const bool inf = p.is_inf();
    if (inf) p = CurveOf<F>::gen();
    Affine<F> r = mul_affine_k256<F>(p, k).to_affine();
    if (inf) r = Affine<F>::inf();
    out[i] = r;
}

static int secret_arg(fk_ctx *ctx, const uint64_t k[4], const char *who, const char *name, Fr *out) {
    if (!k) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null scalar %s", who, name);
    *out = fr_from_limbs(k);
    if (out->is_zero() || !Seedbox::fr_below_modulus(*out)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: %s must be nonzero and its limb image below the modulus", who, name);
    return FK_OK;
}

static int scale_args(fk_ctx *ctx, const void *in, uint64_t n, uint64_t first, const uint64_t x_[4], const uint64_t c_[4], const void *out, Fr *x, Fr *c) {
    if (n && (!in || !out)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "scale_powers: null argument");
    if (first > ~(uint64_t)0 - n) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "scale_powers: first + n passes 2^64");
    if ((n + 63) / 64 > 0x7fffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "scale_powers: n too large");
    FK_TRY(secret_arg(ctx, x_, "scale_powers", "x", x));
    return secret_arg(ctx, c_, "scale_powers", "c", c);
}

template <class F>
static int scale_powers_queue(fk_ctx *ctx, const Affine<F> *d_in, uint64_t n, uint64_t first, const Fr &x, const Fr &c, Affine<F> *d_out) {
    if (!n) return FK_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(powers_scale_kernel<F>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_in, n, first, x, c, d_out);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "powers_scale_kernel");
    return FK_OK;
}

template <class F>
static int scale_powers_dev_entry(fk_ctx *ctx, const void *d_in, uint64_t n, uint64_t first, const uint64_t x_[4], const uint64_t c_[4], void *d_out) {
    if (!ctx) return FK_ERR_BAD_ARG;
    Fr x, c;
    FK_TRY(scale_args(ctx, d_in, n, first, x_, c_, d_out, &x, &c));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return scale_powers_queue<F>(ctx, (const Affine<F> *)d_in, n, first, x, c, (Affine<F> *)d_out);
}

// host arrays through the kernel: staged in stage_a, scaled in place, copied out; blocks
template <class F>
static int scale_powers_staged(fk_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t first, const Fr &x, const Fr &c, uint8_t *out) {
    if (!n) return FK_OK;
    HostStage st{ctx};
    Affine<F> *d = nullptr;
    FK_TRY(st.in(ctx->stage_a, in, n * sizeof(Affine<F>), &d));
    FK_TRY(scale_powers_queue<F>(ctx, d, n, first, x, c, d));
    return st.out(out, d, n * sizeof(Affine<F>));
}

template <class F>
static int scale_powers_entry(fk_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t first, const uint64_t x_[4], const uint64_t c_[4], uint8_t *out) {
    if (!ctx) return host_entry([&](fk_ctx *c0) -> int {
        Fr x, c;
        FK_TRY(scale_args(c0, in, n, first, x_, c_, out, &x, &c));
        host_scale_powers<F>(in, n, first, x, c, out);
        return FK_OK;
    });
    return fk_guard(ctx, [&]() -> int {
        Fr x, c;
        FK_TRY(scale_args(ctx, in, n, first, x_, c_, out, &x, &c));
        FK_TRY(lanes_claim(ctx, "scale_powers"));
        return scale_powers_staged<F>(ctx, in, n, first, x, c, out);
    });
}

// ------------------------------------------------------------------------------------------ contribute
static int contribute_args(fk_ctx *ctx, const fk_powers_desc *in, const uint64_t x_[4], const uint64_t y_[4], const uint64_t z_[4], const fk_powers_out *out,
                           const fk_powers_public *pub, Fr s[3]) {
    const char *who = "powers contribute";
    if (!in || !out || !pub) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    if (!in->tau_g1 || !in->tau_g2 || !in->alpha_tau_g1 || !in->beta_tau_g1 || !in->beta_g2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the transcript lacks an array", who);
    if (!out->tau_g1 || !out->tau_g2 || !out->alpha_tau_g1 || !out->beta_tau_g1 || !out->beta_g2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the output lacks an array", who);
    if (in->n_tau_g1 < 2 || !in->n_tau_g2 || !in->n_alpha_g1 || !in->n_beta_g1)
        FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the transcript is too short: tau_g1 must hold at least 2 elements and the other arrays 1", who);
    const uint64_t longest = std::max(std::max(in->n_tau_g1, in->n_tau_g2), std::max(in->n_alpha_g1, in->n_beta_g1));
    if ((longest + 63) / 64 > 0x7fffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the transcript is too long", who);
    FK_TRY(secret_arg(ctx, x_, who, "x", &s[0]));
    FK_TRY(secret_arg(ctx, y_, who, "y", &s[1]));
    return secret_arg(ctx, z_, who, "z", &s[2]);
}

// beta_g2' and pub: four multiplications in G2 on the host
static void contribute_singles(const fk_powers_desc *in, const Fr s[3], fk_powers_out *out, fk_powers_public *pub) {
    G2Affine b;
    memcpy(&b, in->beta_g2, 128);
    b = host_mul<Fq2>(b, s[2]);
    memcpy(out->beta_g2, &b, 128);
    uint8_t *dst[3] = {pub->x_g2, pub->y_g2, pub->z_g2};
    for (int i = 0; i < 3; i++) {
        const G2Affine p = host_mul<Fq2>(g2_gen(), s[i]);
        memcpy(dst[i], &p, 128);
    }
}

static int contribute_host(fk_ctx *ctx, const fk_powers_desc *in, const uint64_t x_[4], const uint64_t y_[4], const uint64_t z_[4], fk_powers_out *out, fk_powers_public *pub) {
    Fr s[3];
    FK_TRY(contribute_args(ctx, in, x_, y_, z_, out, pub, s));
    const Fr one = Fr::one();
    host_scale_powers<Fq>(in->tau_g1, in->n_tau_g1, 0, s[0], one, out->tau_g1);
    host_scale_powers<Fq2>(in->tau_g2, in->n_tau_g2, 0, s[0], one, out->tau_g2);
    host_scale_powers<Fq>(in->alpha_tau_g1, in->n_alpha_g1, 0, s[0], s[1], out->alpha_tau_g1);
    host_scale_powers<Fq>(in->beta_tau_g1, in->n_beta_g1, 0, s[0], s[2], out->beta_tau_g1);
    contribute_singles(in, s, out, pub);
    return FK_OK;
}

static int contribute_dev(fk_ctx *ctx, const fk_powers_desc *in, const uint64_t x_[4], const uint64_t y_[4], const uint64_t z_[4], fk_powers_out *out, fk_powers_public *pub) {
    Fr s[3];
    FK_TRY(contribute_args(ctx, in, x_, y_, z_, out, pub, s));
    FK_TRY(lanes_claim(ctx, "powers contribute"));
    const Fr one = Fr::one();
    {
        // the longest array first; the single points on the host while its kernel runs
        HostStage st{ctx};
        G1Affine *d = nullptr;
        const size_t bytes = in->n_tau_g1 * sizeof(G1Affine);
        FK_TRY(st.in(ctx->stage_a, in->tau_g1, bytes, &d));
        FK_TRY(scale_powers_queue<Fq>(ctx, d, in->n_tau_g1, 0, s[0], one, d));
        contribute_singles(in, s, out, pub);
        FK_TRY(st.out(out->tau_g1, d, bytes));
    }
    FK_TRY(scale_powers_staged<Fq2>(ctx, in->tau_g2, in->n_tau_g2, 0, s[0], one, out->tau_g2));
    FK_TRY(scale_powers_staged<Fq>(ctx, in->alpha_tau_g1, in->n_alpha_g1, 0, s[0], s[1], out->alpha_tau_g1));
    return scale_powers_staged<Fq>(ctx, in->beta_tau_g1, in->n_beta_g1, 0, s[0], s[2], out->beta_tau_g1);
}

static int powers_new(fk_ctx *ctx, uint64_t m, fk_powers_out *out) {
    if (!out || !out->tau_g1 || !out->tau_g2 || !out->alpha_tau_g1 || !out->beta_tau_g1 || !out->beta_g2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "powers new: null argument");
    if (m < 1 || m >= ((uint64_t)1 << FK_FR_S)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "powers new: m must be at least 1 and below 2^%d", FK_FR_S);
    const G1Affine g1 = g1_gen();
    const G2Affine g2 = g2_gen();
    for (uint64_t i = 0; i < 2 * m - 1; i++) memcpy(out->tau_g1 + 64 * i, &g1, 64);
    for (uint64_t i = 0; i < m; i++) {
        memcpy(out->tau_g2 + 128 * i, &g2, 128);
        memcpy(out->alpha_tau_g1 + 64 * i, &g1, 64);
        memcpy(out->beta_tau_g1 + 64 * i, &g1, 64);
    }
    memcpy(out->beta_g2, &g2, 128);
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ validate points
// One point per lane.  A lane issues atomics only when its point is bad (words_differ_kernel's rule); the lowest bad index is a 64-bit
// atomicMin.  G2: the lanes that are on the curve multiply by r together, digit by digit.
template <class F>
__global__ __launch_bounds__(64) void points_validate_kernel(const Affine<F> *__restrict__ pts, uint64_t n, NafDigits r, PointsCount *rep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = pts[i];
    PointClass c = point_class_on_curve<F>(p);
    if constexpr (CurveOf<F>::HAS_COFACTOR) {
        if (c == PT_GOOD && !mul_naf<F>(p, r).is_inf()) c = PT_SUBGROUP;
    }
    if (c == PT_GOOD) return;
    atomicAdd(c == PT_INFINITY ? &rep->infinity : c == PT_RANGE ? &rep->range : c == PT_CURVE ? &rep->curve : &rep->subgroup, 1ull);
    atomicMin(&rep->first_bad, (unsigned long long)i);
}

// d_rep is cleared (counts 0, first_bad all ones) and filled, all on the stream
template <class F>
static int validate_queue(fk_ctx *ctx, const Affine<F> *d_pts, uint64_t n, PointsCount *d_rep) {
    if ((n + 63) / 64 > 0x7fffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "points validate: n too large");
    FK_HIP(ctx, hipMemsetAsync(d_rep, 0, offsetof(PointsCount, first_bad), ctx->stream));
    FK_HIP(ctx, hipMemsetAsync(&d_rep->first_bad, 0xff, sizeof(d_rep->first_bad), ctx->stream));
    if (!n) return FK_OK;
    const NafDigits r = naf_recode(r_as_limbs());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(points_validate_kernel<F>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_pts, n, r, d_rep);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "points_validate_kernel");
    return FK_OK;
}

static void report_of(const PointsCount &c, fk_points_report *rep) {
    rep->infinity = c.infinity; rep->range = c.range; rep->curve = c.curve; rep->subgroup = c.subgroup; rep->first_bad = c.first_bad;
}
static bool report_clean(const fk_points_report &r) { return !(r.infinity | r.range | r.curve | r.subgroup); }

static int validate_host(fk_ctx *c, const uint8_t *pts, uint64_t n, int g2, fk_points_report *rep) {
    if (!rep || (n && !pts)) FK_SET_ERR(c, FK_ERR_BAD_ARG, "points validate: null argument");
    if (g2 != 0 && g2 != 1) FK_SET_ERR(c, FK_ERR_BAD_ARG, "points validate: g2 must be 0 or 1");
    PointsCount cnt;
    if (g2) host_points_validate<Fq2>(pts, n, &cnt); else host_points_validate<Fq>(pts, n, &cnt);
    report_of(cnt, rep);
    return FK_OK;
}

// the report slots of a call live at the head of ctx->misc
static constexpr size_t VALIDATE_SLOTS = 4;

static int validate_staged(fk_ctx *ctx, const uint8_t *pts, uint64_t n, int g2, fk_points_report *rep) {
    if (!rep || (n && !pts)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "points validate: null argument");
    if (g2 != 0 && g2 != 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "points validate: g2 must be 0 or 1");
    FK_TRY(lanes_claim(ctx, "points validate"));
    FK_HIP(ctx, ctx->misc.reserve(VALIDATE_SLOTS * sizeof(PointsCount)));
    PointsCount *d_rep = ctx->misc.as<PointsCount>();
    HostStage st{ctx};
    if (g2) {
        G2Affine *d = nullptr;
        FK_TRY(st.in(ctx->stage_a, pts, n * sizeof(G2Affine), &d));
        FK_TRY(validate_queue<Fq2>(ctx, d, n, d_rep));
    } else {
        G1Affine *d = nullptr;
        FK_TRY(st.in(ctx->stage_a, pts, n * sizeof(G1Affine), &d));
        FK_TRY(validate_queue<Fq>(ctx, d, n, d_rep));
    }
    PointsCount cnt;
    FK_TRY(st.out(&cnt, d_rep, sizeof cnt));
    report_of(cnt, rep);
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ check an update
struct UpdateView {            // the prefixes a domain of m uses
    const uint8_t *arr[4];     // tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1
    uint64_t len[4];
    const uint8_t *beta_g2;
};
static constexpr int ARR_G2 = 1;      // the one G2 array of UpdateView::arr

static int update_view(fk_ctx *ctx, const fk_powers_desc *p, uint64_t m, const char *which, UpdateView *v, bool *long_enough) {
    if (!p) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "powers update check: null transcript (%s)", which);
    if (!p->tau_g1 || !p->tau_g2 || !p->alpha_tau_g1 || !p->beta_tau_g1 || !p->beta_g2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "powers update check: the transcript (%s) lacks an array", which);
    *v = UpdateView{{p->tau_g1, p->tau_g2, p->alpha_tau_g1, p->beta_tau_g1}, {2 * m - 1, m, m, m}, p->beta_g2};
    *long_enough = p->n_tau_g1 >= 2 * m - 1 && p->n_tau_g2 >= m && p->n_alpha_g1 >= m && p->n_beta_g1 >= m;
    return FK_OK;
}

template <class F>
static Affine<F> point_at(const uint8_t *arr, uint64_t i) {
    Affine<F> p;
    memcpy(&p, arr + sizeof(Affine<F>) * i, sizeof p);
    return p;
}
// a point no pairing may read: not a pair of field elements, or not on the curve
template <class F>
static bool unpairable(const Affine<F> &p) {
    const PointClass c = point_class_on_curve<F>(p);
    return c == PT_RANGE || c == PT_CURVE;
}

// `dev`: through the kernels of ctx; otherwise the host references (ctx then only carries the message)
static int update_check(fk_ctx *ctx, bool dev, const fk_powers_desc *before, const fk_powers_desc *after, const fk_powers_public *pub, uint64_t m, const uint8_t *seed,
                        fk_powers_update_report *rep) {
    const char *who = "powers update check";
    if (!pub || !rep || (!dev && !seed)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null argument", who);
    if (m < 2 || m >= ((uint64_t)1 << FK_FR_S)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: m must be at least 2 and below 2^%d", who, FK_FR_S);
    UpdateView vb, va;
    bool long_b = false, long_a = false;
    FK_TRY(update_view(ctx, before, m, "before", &vb, &long_b));
    FK_TRY(update_view(ctx, after, m, "after", &va, &long_a));
    if (dev) FK_TRY(lanes_claim(ctx, who));
    memset(rep, 0, sizeof *rep);
    fk_points_report *reports[5] = {&rep->tau_g1, &rep->tau_g2, &rep->alpha_tau_g1, &rep->beta_tau_g1, &rep->beta_g2};
    for (fk_points_report *r : reports) r->first_bad = ~(uint64_t)0;
    rep->shape_ok = long_b && long_a;
    if (!rep->shape_ok) return FK_OK;

    // ---- the points of `after`
    if (dev) {
        FK_HIP(ctx, ctx->misc.reserve(VALIDATE_SLOTS * sizeof(PointsCount)));
        PointsCount *d_rep = ctx->misc.as<PointsCount>();
        HostStage st{ctx};
        for (int k = 0; k < 4; k++) {          // one array after another through stage_a: the stream keeps kernel k in front of copy k + 1
            if (k == ARR_G2) {
                G2Affine *d = nullptr;
                FK_TRY(st.in(ctx->stage_a, va.arr[k], va.len[k] * sizeof(G2Affine), &d));
                FK_TRY(validate_queue<Fq2>(ctx, d, va.len[k], d_rep + k));
            } else {
                G1Affine *d = nullptr;
                FK_TRY(st.in(ctx->stage_a, va.arr[k], va.len[k] * sizeof(G1Affine), &d));
                FK_TRY(validate_queue<Fq>(ctx, d, va.len[k], d_rep + k));
            }
        }
        PointsCount cnt[VALIDATE_SLOTS];
        FK_TRY(st.out(cnt, d_rep, sizeof cnt));
        for (int k = 0; k < 4; k++) report_of(cnt[k], reports[k]);
    } else {
        for (int k = 0; k < 4; k++) {
            PointsCount cnt;
            if (k == ARR_G2) host_points_validate<Fq2>(va.arr[k], va.len[k], &cnt); else host_points_validate<Fq>(va.arr[k], va.len[k], &cnt);
            report_of(cnt, reports[k]);
        }
    }
    {
        PointsCount cnt;
        host_points_validate<Fq2>(va.beta_g2, 1, &cnt);      // an array of one: on the host either way
        report_of(cnt, reports[4]);
    }
    rep->points_ok = 1;
    for (const fk_points_report *r : reports) rep->points_ok &= report_clean(*r);

    // ---- the transcript check on `after`
    if (dev) {
        FK_TRY(fk_powers_check(ctx, after, m, seed, &rep->after));
    } else {
        const int rc = fk_powers_check_host(after, m, seed, &rep->after);
        if (rc != FK_OK) { ctx->err = tls_error(); return rc; }
    }

    // ---- the single points the pairings read; nothing with a range or curve failure is paired
    const G1Affine a_tau1 = point_at<Fq>(va.arr[0], 1), a_alpha0 = point_at<Fq>(va.arr[2], 0), a_beta0 = point_at<Fq>(va.arr[3], 0);
    const G1Affine b_tau1 = point_at<Fq>(vb.arr[0], 1), b_alpha0 = point_at<Fq>(vb.arr[2], 0), b_beta0 = point_at<Fq>(vb.arr[3], 0);
    const G2Affine a_tau2_1 = point_at<Fq2>(va.arr[1], 1), a_beta_g2 = point_at<Fq2>(va.beta_g2, 0);
    const G2Affine x_g2 = point_at<Fq2>(pub->x_g2, 0), y_g2 = point_at<Fq2>(pub->y_g2, 0), z_g2 = point_at<Fq2>(pub->z_g2, 0);
    fk_powers_report &ar = rep->after;
    if (unpairable(a_tau1)) ar.tau_pair = ar.ratio_tau_g2 = 0;
    if (unpairable(a_tau2_1)) ar.tau_pair = ar.ratio_tau_g1 = ar.ratio_alpha = ar.ratio_beta = 0;
    if (unpairable(a_beta0) || unpairable(a_beta_g2)) ar.beta_pair = 0;
    auto unsummed = [](const fk_points_report &r, int32_t &flag, uint8_t *s, uint8_t *s_next, size_t bytes) {
        if (!(r.range | r.curve)) return;
        flag = 0; memset(s, 0, bytes); memset(s_next, 0, bytes);
    };
    unsummed(rep->tau_g1, ar.ratio_tau_g1, ar.s_tau_g1, ar.s_tau_g1_next, 64);
    unsummed(rep->tau_g2, ar.ratio_tau_g2, ar.s_tau_g2, ar.s_tau_g2_next, 128);
    unsummed(rep->alpha_tau_g1, ar.ratio_alpha, ar.s_alpha, ar.s_alpha_next, 64);
    unsummed(rep->beta_tau_g1, ar.ratio_beta, ar.s_beta, ar.s_beta_next, 64);
    ar.accept = ar.gen_ok && ar.tau_pair && ar.ratio_tau_g1 && ar.ratio_tau_g2 && ar.ratio_alpha && ar.ratio_beta && ar.beta_pair;

    // ---- the steps
    const G2Affine g2 = g2_gen();
    auto step = [&](const G1Affine &a, const G1Affine &b, const G2Affine &s) -> int32_t {
        if (unpairable(a) || unpairable(b) || unpairable(s)) return 0;
        return pairing_eq(a, g2, b, s);
    };
    rep->step_tau = step(a_tau1, b_tau1, x_g2);
    rep->step_alpha = step(a_alpha0, b_alpha0, y_g2);
    rep->step_beta = step(a_beta0, b_beta0, z_g2);
    rep->changed = memcmp(&a_tau1, &b_tau1, 64) != 0;
    rep->accept = rep->shape_ok && rep->points_ok && ar.accept && rep->step_tau && rep->step_alpha && rep->step_beta;
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_g1_scale_powers_dev(fk_ctx *ctx, const void *d_in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], void *d_out) {
    return fk_guard(ctx, [&]() -> int { return scale_powers_dev_entry<Fq>(ctx, d_in, n, first, x, c, d_out); });
}
int fk_g2_scale_powers_dev(fk_ctx *ctx, const void *d_in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], void *d_out) {
    return fk_guard(ctx, [&]() -> int { return scale_powers_dev_entry<Fq2>(ctx, d_in, n, first, x, c, d_out); });
}
int fk_g1_scale_powers(fk_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], uint8_t *out) {
    return scale_powers_entry<Fq>(ctx, in, n, first, x, c, out);
}
int fk_g2_scale_powers(fk_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], uint8_t *out) {
    return scale_powers_entry<Fq2>(ctx, in, n, first, x, c, out);
}

int fk_powers_new(uint64_t m, fk_powers_out *out) { return host_entry([&](fk_ctx *c) -> int { return powers_new(c, m, out); }); }

int fk_powers_contribute(fk_ctx *ctx, const fk_powers_desc *in, const uint64_t x[4], const uint64_t y[4], const uint64_t z[4], fk_powers_out *out, fk_powers_public *pub) {
    return fk_guard(ctx, [&]() -> int {
        FK_RANGE("fk_powers_contribute");
        if (!ctx) return FK_ERR_BAD_ARG;
        return contribute_dev(ctx, in, x, y, z, out, pub);
    });
}
int fk_powers_contribute_host(const fk_powers_desc *in, const uint64_t x[4], const uint64_t y[4], const uint64_t z[4], fk_powers_out *out, fk_powers_public *pub) {
    return host_entry([&](fk_ctx *c) -> int { return contribute_host(c, in, x, y, z, out, pub); });
}

int fk_points_validate(fk_ctx *ctx, const uint8_t *pts, uint64_t n, int g2, fk_points_report *rep) {
    if (!ctx) return host_entry([&](fk_ctx *c) -> int { return validate_host(c, pts, n, g2, rep); });
    return fk_guard(ctx, [&]() -> int { return validate_staged(ctx, pts, n, g2, rep); });
}
int fk_points_validate_dev(fk_ctx *ctx, const void *d_pts, uint64_t n, int g2, void *d_rep) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!d_rep || (n && !d_pts) || ((uintptr_t)d_rep & 7)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "points validate: null or misaligned argument");
    if (g2 != 0 && g2 != 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "points validate: g2 must be 0 or 1");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return g2 ? validate_queue<Fq2>(ctx, (const G2Affine *)d_pts, n, (PointsCount *)d_rep) : validate_queue<Fq>(ctx, (const G1Affine *)d_pts, n, (PointsCount *)d_rep);
}); }

int fk_powers_update_check(fk_ctx *ctx, const fk_powers_desc *before, const fk_powers_desc *after, const fk_powers_public *pub, uint64_t m,
                           const uint8_t *seed, fk_powers_update_report *rep) {
    return fk_guard(ctx, [&]() -> int {
        FK_RANGE("fk_powers_update_check");
        if (!ctx) return FK_ERR_BAD_ARG;
        return update_check(ctx, true, before, after, pub, m, seed, rep);
    });
}
int fk_powers_update_check_host(const fk_powers_desc *before, const fk_powers_desc *after, const fk_powers_public *pub, uint64_t m,
                                const uint8_t seed[32], fk_powers_update_report *rep) {
    return host_entry([&](fk_ctx *c) -> int { return update_check(c, false, before, after, pub, m, seed, rep); });
}

}  // extern "C"
