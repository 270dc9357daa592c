// Key ceremony, phase 2 (include/fawkes_hip_ceremony.h): apply one delta contribution to a proving key, and check one.
//
// Contribute: h' = [1/x] h, l' = [1/x] l -- n_h + n_l multiplications of a point by ONE scalar (g1_scale_kernel); the two deltas times x on
// the host; a, b_g1, b_g2 copied device to device.  Check: four multi-scalar multiplications with 128-bit weights from a ChaCha20 stream
// (weights_kernel; the existing MSM over the keys' own arrays), a word compare of the fixed arrays (words_differ_kernel), six Miller
// loops and three final exponentiations on the host (pairing.hpp).  The host entries are the plain references the device is compared with.
#include "ceremony_shared.hpp"   // generators, pairing_eq, lanes_claim, draw_seed, host_entry
#include "poseidon.hpp"          // chacha20_block, Seedbox::fr_below_modulus, fr_from_limbs
#include "../../include/fawkes_hip_ceremony.h"
#include <memory>

namespace fk {

// ------------------------------------------------------------------------------------------ one scalar, many points
// (NafDigits, naf_recode and mul_naf live in ceremony_shared.hpp: powers.hip walks r with them)
// One point per lane.  A lane whose input is the point at infinity runs the loop on the generator and stores infinity: it stays in step
// with its wave instead of making all 64 lanes wait for two paths through ~340 group operations.  in == out is allowed (a lane reads its
// own element before it writes it), hence no __restrict__.
__global__ __launch_bounds__(64) void g1_scale_kernel(const G1Affine *in, size_t n, NafDigits k, G1Affine *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine p = in[i];
    const bool inf = p.is_inf() || k.n == 0;
    if (inf) { p.x = Fq::one(); p.y = Fq::dbl(Fq::one()); }
    G1Affine r = mul_naf<Fq>(p, k).to_affine();
    if (inf) r = G1Affine::inf();
    out[i] = r;
}

static int scalar_arg(fk_ctx *ctx, const uint64_t k[4], const char *who, Fr *out) {
    if (!k) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null scalar", who);
    *out = fr_from_limbs(k);
    if (!Seedbox::fr_below_modulus(*out)) FK_SET_ERR(ctx, FK_ERR_FORMAT, "%s: the scalar's limb image is not below the modulus", who);
    return FK_OK;
}

static int g1_scale_queue(fk_ctx *ctx, const G1Affine *d_in, size_t n, const Fr &k_mont, G1Affine *d_out) {
    if (!n) return FK_OK;
    const size_t blocks = (n + 63) / 64;
    if (blocks > 0x7fffffffull) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "g1_scale: n too large");
    const NafDigits d = naf_recode(Fr::from_mont(k_mont));
    hipLaunchKernelGGL(g1_scale_kernel, dim3((unsigned)blocks), dim3(64), 0, ctx->stream, d_in, n, d, d_out);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "g1_scale_kernel");
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ the weights
struct SeedWords { uint32_t w[8]; };
static SeedWords seed_words(const uint8_t seed[32]) {
    SeedWords s;
    for (int i = 0; i < 8; i++) s.w[i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 | (uint32_t)seed[4 * i + 3] << 24;
    return s;
}
// four words of a block -> the weight, Montgomery; a zero draw becomes 1
static FK_HD Fr weight_mont(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    if (!(w0 | w1 | w2 | w3)) w0 = 1;
    Fr r = Fr::zero();
    r.v[0] = w0; r.v[1] = w1; r.v[2] = w2; r.v[3] = w3;
    return Fr::to_mont(r);
}

// one ChaCha20 block, i.e. four weights, per lane
__global__ __launch_bounds__(256) void weights_kernel(SeedWords key, size_t n, Fr *__restrict__ out) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * b >= n) return;
    uint32_t blk[16];
    chacha20_block(key.w, b, 0, blk);
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (4 * b + j < n) out[4 * b + j] = weight_mont(blk[4 * j], blk[4 * j + 1], blk[4 * j + 2], blk[4 * j + 3]);
}

static int weights_queue(fk_ctx *ctx, const uint8_t seed[32], size_t n, Fr *d_out) {
    if (!n) return FK_OK;
    const size_t blocks = ((n + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(weights_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, seed_words(seed), n, d_out);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "weights_kernel");
    return FK_OK;
}

// the raw 128-bit weights (lo, hi) the host sums multiply by, and their Montgomery images
static void weights_host(const uint8_t seed[32], size_t n, uint64_t *raw, Fr *mont) {
    const SeedWords key = seed_words(seed);
    uint32_t blk[16];
    for (size_t i = 0; i < n; i++) {
        if (!(i & 3)) chacha20_block(key.w, i >> 2, 0, blk);
        const uint32_t *w = blk + 4 * (i & 3);
        if (mont) mont[i] = weight_mont(w[0], w[1], w[2], w[3]);
        if (raw) {
            raw[2 * i] = (uint64_t)w[0] | (uint64_t)w[1] << 32; raw[2 * i + 1] = (uint64_t)w[2] | (uint64_t)w[3] << 32;
            if (!(raw[2 * i] | raw[2 * i + 1])) raw[2 * i] = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------ the check
// flag |= OR of a[i] ^ b[i] over n 64-bit words: zero iff the arrays are equal
__global__ __launch_bounds__(256) void words_differ_kernel(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, size_t n, unsigned long long *flag) {
    uint64_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc |= a[i] ^ b[i];
    if (acc) atomicOr(flag, (unsigned long long)acc);
}

// what a check reads of one key besides its arrays
struct KeyHead {
    uint64_t m, num_input, num_aux, n_h, n_l, n_a, n_b;
    G1Affine alpha_g1, beta_g1, delta_g1;
    G2Affine beta_g2, delta_g2;
};
static KeyHead head_of(const fk_key *k) {
    return KeyHead{k->m, k->num_input, k->num_aux, k->n_h, k->n_l, k->n_a, k->n_b, k->alpha_g1, k->beta_g1, k->delta_g1, k->beta_g2, k->delta_g2};
}
static KeyHead head_of(const fk_key_desc *d) {
    KeyHead h{d->m, d->num_input, d->num_aux, d->n_h, d->n_l, d->n_a, d->n_b, {}, {}, {}, {}, {}};
    memcpy(&h.alpha_g1, d->alpha_g1, 64); memcpy(&h.beta_g1, d->beta_g1, 64); memcpy(&h.delta_g1, d->delta_g1, 64);
    memcpy(&h.beta_g2, d->beta_g2, 128); memcpy(&h.delta_g2, d->delta_g2, 128);
    return h;
}
static bool same_shape(const KeyHead &a, const KeyHead &b) {
    return a.m == b.m && a.num_input == b.num_input && a.num_aux == b.num_aux && a.n_h == b.n_h && a.n_l == b.n_l && a.n_a == b.n_a && a.n_b == b.n_b;
}

// The verdict from the two heads, whether a, b_g1, b_g2 were found equal, and the four sums S_h, S_h', S_l, S_l' (shape_equal only).
static void verdict(const KeyHead &b, const KeyHead &a, bool shape_equal, bool arrays_equal, const G1Affine s[4], const uint8_t seed[32], fk_contribution_report *rep) {
    memset(rep, 0, sizeof *rep);
    memcpy(rep->seed, seed, 32);
    rep->shape_equal = shape_equal;
    rep->delta_nonzero = !a.delta_g1.is_inf() && !a.delta_g2.is_inf();
    rep->delta_pair = pairing_eq(a.delta_g1, g2_gen(), g1_gen(), a.delta_g2);
    rep->delta_changed = memcmp(&a.delta_g1, &b.delta_g1, 64) != 0;
    if (shape_equal) {
        rep->fixed_equal = arrays_equal && !memcmp(&a.alpha_g1, &b.alpha_g1, 64) && !memcmp(&a.beta_g1, &b.beta_g1, 64) && !memcmp(&a.beta_g2, &b.beta_g2, 128);
        rep->ratio_h = pairing_eq(s[1], a.delta_g2, s[0], b.delta_g2);
        rep->ratio_l = pairing_eq(s[3], a.delta_g2, s[2], b.delta_g2);
        memcpy(rep->s_h, &s[0], 64); memcpy(rep->s_h_after, &s[1], 64); memcpy(rep->s_l, &s[2], 64); memcpy(rep->s_l_after, &s[3], 64);
    }
    rep->accept = rep->shape_equal && rep->fixed_equal && rep->delta_nonzero && rep->delta_pair && rep->ratio_h && rep->ratio_l;
}

static int desc_ok(fk_ctx *ctx, const fk_key_desc *d, const char *who) {
    if (!d) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null key description", who);
    if (d->shard_count != 1 || d->shard_index != 0) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a sharded key (shard %u of %u): the ceremony works on whole keys", who, d->shard_index, d->shard_count);
    if (!d->alpha_g1 || !d->beta_g1 || !d->delta_g1 || !d->beta_g2 || !d->delta_g2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: missing vk points", who);
    if ((d->n_h && !d->h) || (d->n_l && !d->l) || (d->n_a && !d->a) || (d->n_b && (!d->b_g1 || !d->b_g2))) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: missing key array", who);
    return FK_OK;
}

// a whole key resident on ctx's device
static int key_ok(fk_ctx *ctx, const fk_key *k, const char *who) {
    if (!k || !k->d_h || !k->d_l || !k->d_a || !k->d_b1 || !k->d_b2) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: null key, or a key without device arrays", who);
    if (k->shard_count != 1) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a sharded key (shard %u of %u): the ceremony works on whole keys", who, k->shard_index, k->shard_count);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, k->d_h) != hipSuccess) { (void)hipGetLastError(); FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the key's arrays are not device memory", who); }
    if (at.device != ctx->device) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: the key is resident on device %d, the context is on device %d", who, at.device, ctx->device);
    return FK_OK;
}

static int check_host(fk_ctx *ctx, const fk_key_desc *before, const fk_key_desc *after, const uint8_t *seed, fk_contribution_report *report) {
    if (!seed || !report) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribution check: null argument");
    FK_TRY(desc_ok(ctx, before, "contribution check (before)"));
    FK_TRY(desc_ok(ctx, after, "contribution check (after)"));
    const KeyHead hb = head_of(before), ha = head_of(after);
    const bool shape = same_shape(hb, ha);
    bool arrays = false;
    G1Affine s[4] = {G1Affine::inf(), G1Affine::inf(), G1Affine::inf(), G1Affine::inf()};
    if (shape) {
        arrays = (!hb.n_a || !memcmp(before->a, after->a, hb.n_a * 64)) && (!hb.n_b || (!memcmp(before->b_g1, after->b_g1, hb.n_b * 64) && !memcmp(before->b_g2, after->b_g2, hb.n_b * 128)));
        const size_t nw = (size_t)(hb.n_h > hb.n_l ? hb.n_h : hb.n_l);
        std::vector<uint64_t> w(2 * nw);
        weights_host(seed, nw, w.data(), nullptr);
        auto sum = [&](const uint8_t *pts, uint64_t n) {
            G1Xyzz acc = G1Xyzz::inf();
            for (uint64_t i = 0; i < n; i++) {
                G1Affine p;
                memcpy(&p, pts + 64 * i, 64);
                acc.add(G1Xyzz::mul_affine_bits(p, w[2 * i], w[2 * i + 1], 128));
            }
            return acc.to_affine();
        };
        s[0] = sum(before->h, hb.n_h); s[1] = sum(after->h, hb.n_h); s[2] = sum(before->l, hb.n_l); s[3] = sum(after->l, hb.n_l);
    }
    verdict(hb, ha, shape, arrays, s, seed, report);
    return FK_OK;
}

static int check_dev(fk_ctx *ctx, const fk_key *before, const fk_key *after, const uint8_t *seed_in, fk_contribution_report *report) {
    if (!report) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribution check: null argument");
    FK_TRY(lanes_claim(ctx, "contribution check"));
    FK_TRY(key_ok(ctx, before, "contribution check (before)"));
    FK_TRY(key_ok(ctx, after, "contribution check (after)"));
    uint8_t seed[32];
    if (seed_in) memcpy(seed, seed_in, 32); else FK_TRY(draw_seed(ctx, seed, "contribution check"));
    const KeyHead hb = head_of(before), ha = head_of(after);
    const bool shape = same_shape(hb, ha);
    bool arrays = false;
    G1Affine s[4] = {G1Affine::inf(), G1Affine::inf(), G1Affine::inf(), G1Affine::inf()};
    if (shape) {
        // a, b_g1, b_g2: one word says whether anything differs.  Queued first: it runs underneath the first multiplication's sort.
        FK_HIP(ctx, ctx->misc.reserve(8));
        unsigned long long *d_flag = ctx->misc.as<unsigned long long>();
        FK_HIP(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
        auto differ = [&](const void *x, const void *y, size_t bytes) {
            const size_t words = bytes / 8;
            if (!words) return;
            const size_t blocks = (words + 255) / 256;
            hipLaunchKernelGGL(words_differ_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, ctx->stream, (const uint64_t *)x, (const uint64_t *)y, words, d_flag);
        };
        differ(before->d_a, after->d_a, hb.n_a * 64); differ(before->d_b1, after->d_b1, hb.n_b * 64); differ(before->d_b2, after->d_b2, hb.n_b * 128);
        FK_HIP(ctx, hipGetLastError());
        FK_DBG(ctx, "words_differ_kernel");
        // the weights once, for the longer of h and l; the four sums over the keys' own arrays
        const size_t nw = (size_t)(hb.n_h > hb.n_l ? hb.n_h : hb.n_l);
        FK_HIP(ctx, ctx->ceremony.reserve(nw * sizeof(Fr)));
        Fr *d_w = ctx->ceremony.as<Fr>();
        FK_TRY(weights_queue(ctx, seed, nw, d_w));
        const G1Affine *arr[4] = {before->d_h, after->d_h, before->d_l, after->d_l};
        for (int i = 0; i < 4; i++) {
            G1Xyzz r;
            FK_TRY(msm_g1_dev(ctx, arr[i], d_w, (size_t)(i < 2 ? hb.n_h : hb.n_l), &r));
            s[i] = r.to_affine();
        }
        unsigned long long flag = 1;
        FK_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        arrays = flag == 0;
    }
    verdict(hb, ha, shape, arrays, s, seed, report);
    return FK_OK;
}

static int contribute_host(fk_ctx *ctx, const fk_key_desc *in, const uint64_t x_[4], uint8_t *h_out, uint8_t *l_out, uint8_t *delta_g1_out, uint8_t *delta_g2_out) {
    FK_TRY(desc_ok(ctx, in, "contribute"));
    if ((in->n_h && !h_out) || (in->n_l && !l_out) || !delta_g1_out || !delta_g2_out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribute: null output");
    Fr x;
    FK_TRY(scalar_arg(ctx, x_, "contribute", &x));
    if (x.is_zero()) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribute: x must not be zero");
    const Fr xi = Fr::inv(x);
    auto scale = [&](const uint8_t *pts, uint64_t n, uint8_t *out) {
        for (uint64_t i = 0; i < n; i++) {
            G1Affine p;
            memcpy(&p, pts + 64 * i, 64);
            p = host_mul<Fq>(p, xi);
            memcpy(out + 64 * i, &p, 64);
        }
    };
    scale(in->h, in->n_h, h_out); scale(in->l, in->n_l, l_out);
    const KeyHead h = head_of(in);
    const G1Affine d1 = host_mul<Fq>(h.delta_g1, x);
    const G2Affine d2 = host_mul<Fq2>(h.delta_g2, x);
    memcpy(delta_g1_out, &d1, 64); memcpy(delta_g2_out, &d2, 128);
    return FK_OK;
}

static int contribute_dev(fk_ctx *ctx, const fk_key *key, const uint64_t x_[4], uint32_t flags, fk_key **out_key) {
    if (!out_key) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribute: null argument");
    *out_key = nullptr;
    if (flags & ~(uint32_t)FK_KEY_NO_LEVELS) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribute: flags must be 0 or FK_KEY_NO_LEVELS");
    Fr x;
    FK_TRY(scalar_arg(ctx, x_, "contribute", &x));
    if (x.is_zero()) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "contribute: x must not be zero");
    FK_TRY(lanes_claim(ctx, "contribute"));
    FK_TRY(key_ok(ctx, key, "contribute"));
    auto drop = [ctx](fk_key *k) { fk_key_free(ctx, k); };
    std::unique_ptr<fk_key, decltype(drop)> k(new fk_key(), drop);
    k->m = key->m; k->num_input = key->num_input; k->num_aux = key->num_aux;
    k->n_h = key->n_h; k->n_l = key->n_l; k->n_a = key->n_a; k->n_b = key->n_b;
    FK_TRY(key_plan_slices(ctx, k.get(), FK_Z_EQUAL_SPLIT, FK_Z_EQUAL_SPLIT));
    // the arrays as setup_impl and the bellman loader allocate them: one spare element each
    FK_HIP(ctx, hipMalloc((void **)&k->d_h, (k->n_h + 1) * sizeof(G1Affine)));
    FK_HIP(ctx, hipMalloc((void **)&k->d_l, (k->n_l + 1) * sizeof(G1Affine)));
    FK_HIP(ctx, hipMalloc((void **)&k->d_a, (k->n_a + 1) * sizeof(G1Affine)));
    FK_HIP(ctx, hipMalloc((void **)&k->d_b1, (k->n_b + 1) * sizeof(G1Affine)));
    FK_HIP(ctx, hipMalloc((void **)&k->d_b2, (k->n_b + 1) * sizeof(G2Affine)));
    if (k->n_a) FK_HIP(ctx, hipMemcpyAsync(k->d_a, key->d_a, k->n_a * sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
    if (k->n_b) FK_HIP(ctx, hipMemcpyAsync(k->d_b1, key->d_b1, k->n_b * sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
    if (k->n_b) FK_HIP(ctx, hipMemcpyAsync(k->d_b2, key->d_b2, k->n_b * sizeof(G2Affine), hipMemcpyDeviceToDevice, ctx->stream));
    const Fr xi = Fr::inv(x);
    FK_TRY(g1_scale_queue(ctx, key->d_h, (size_t)k->n_h, xi, k->d_h));
    FK_TRY(g1_scale_queue(ctx, key->d_l, (size_t)k->n_l, xi, k->d_l));
    k->alpha_g1 = key->alpha_g1; k->beta_g1 = key->beta_g1; k->beta_g2 = key->beta_g2;
    k->delta_g1 = host_mul<Fq>(key->delta_g1, x);          // (while the kernels run)
    k->delta_g2 = host_mul<Fq2>(key->delta_g2, x);
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!(flags & FK_KEY_NO_LEVELS)) FK_TRY(key_precompute(ctx, k.get()));
    *out_key = k.release();
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_g1_scale_dev(fk_ctx *ctx, const void *d_in, size_t n, const uint64_t k[4], void *d_out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (n && (!d_in || !d_out)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "g1_scale: null argument");
    Fr km;
    FK_TRY(scalar_arg(ctx, k, "g1_scale", &km));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return g1_scale_queue(ctx, (const G1Affine *)d_in, n, km, (G1Affine *)d_out);
}); }

int fk_g1_scale(fk_ctx *ctx, const uint8_t *in, size_t n, const uint64_t k[4], uint8_t *out) {
    if (!ctx) return host_entry([&](fk_ctx *c) -> int {
        if (n && (!in || !out)) FK_SET_ERR(c, FK_ERR_BAD_ARG, "g1_scale: null argument");
        Fr km;
        FK_TRY(scalar_arg(c, k, "g1_scale", &km));
        for (size_t i = 0; i < n; i++) {
            G1Affine p;
            memcpy(&p, in + 64 * i, 64);
            p = host_mul<Fq>(p, km);
            memcpy(out + 64 * i, &p, 64);
        }
        return FK_OK;
    });
    return fk_guard(ctx, [&]() -> int {
        if (n && (!in || !out)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "g1_scale: null argument");
        Fr km;
        FK_TRY(scalar_arg(ctx, k, "g1_scale", &km));
        FK_TRY(scratch_claim(ctx, "g1_scale"));
        if (!n) return FK_OK;
        HostStage st{ctx};
        G1Affine *d = nullptr;
        FK_TRY(st.in(ctx->stage_a, in, n * sizeof(G1Affine), &d));
        FK_TRY(g1_scale_queue(ctx, d, n, km, d));
        return st.out(out, d, n * sizeof(G1Affine));
    });
}

int fk_key_contribute(fk_ctx *ctx, const fk_key *key, const uint64_t x[4], uint32_t flags, fk_key **out_key) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_key_contribute");
    if (!ctx) return FK_ERR_BAD_ARG;
    return contribute_dev(ctx, key, x, flags, out_key);
}); }

int fk_key_contribute_host(const fk_key_desc *in, const uint64_t x[4], uint8_t *h_out, uint8_t *l_out, uint8_t *delta_g1_out, uint8_t *delta_g2_out) {
    return host_entry([&](fk_ctx *c) -> int { return contribute_host(c, in, x, h_out, l_out, delta_g1_out, delta_g2_out); });
}

int fk_ceremony_weights(const uint8_t seed[32], size_t n, uint64_t *out) {
    return host_entry([&](fk_ctx *c) -> int {
        if (!seed || (n && !out)) FK_SET_ERR(c, FK_ERR_BAD_ARG, "ceremony weights: null argument");
        static_assert(sizeof(Fr) == 32, "a weight is four limbs");
        weights_host(seed, n, nullptr, (Fr *)out);
        return FK_OK;
    });
}

int fk_ceremony_weights_dev(fk_ctx *ctx, const uint8_t seed[32], size_t n, void *d_out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!seed || (n && !d_out)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "ceremony weights: null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return weights_queue(ctx, seed, n, (Fr *)d_out);
}); }

int fk_key_contribution_check(fk_ctx *ctx, const fk_key *before, const fk_key *after, const uint8_t *seed, fk_contribution_report *report) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_key_contribution_check");
    if (!ctx) return FK_ERR_BAD_ARG;
    return check_dev(ctx, before, after, seed, report);
}); }

int fk_key_contribution_check_host(const fk_key_desc *before, const fk_key_desc *after, const uint8_t seed[32], fk_contribution_report *report) {
    return host_entry([&](fk_ctx *c) -> int { return check_host(c, before, after, seed, report); });
}

}  // extern "C"
