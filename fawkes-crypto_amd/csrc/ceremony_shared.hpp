// What ceremony.hip (one phase-2 step), ceremony_init.hip (the initial key from a powers-of-tau transcript) and powers.hip (phase 1) share.
// On the host: the generators, the pairing comparison of a check, the seed of its weights, the claim of a device entry and the frame of a
// host-only entry.  On host and device: a point times one scalar for all lanes (NafDigits, mul_naf) and times the lane's own (K256).
#pragma once
#include "common.hpp"
#include "pairing.hpp"
#include <sys/random.h>
#include <errno.h>
#include <string.h>

namespace fk {

static inline G1Affine g1_gen() { return G1Affine{Fq::one(), Fq::dbl(Fq::one())}; }
static inline G2Affine g2_gen() {
    const uint32_t x0[8] = FK_G2_GEN_X0, x1[8] = FK_G2_GEN_X1, y0[8] = FK_G2_GEN_Y0, y1[8] = FK_G2_GEN_Y1;
    G2Affine g;
    for (int i = 0; i < 8; i++) { g.x.c0.v[i] = x0[i]; g.x.c1.v[i] = x1[i]; g.y.c0.v[i] = y0[i]; g.y.c1.v[i] = y1[i]; }
    return g;
}

// e(p1, q1) == e(p2, q2); a pairing with the point at infinity on either side is one
static inline bool pairing_eq(const G1Affine &p1, const G2Affine &q1, const G1Affine &p2, const G2Affine &q2) {
    using F12 = Fq12T<Fq>;
    const F12 m = F12::mul(miller_loop_proj<Fq>(p1, q1), miller_loop_proj<Fq>(affine_neg_if(p2, true), q2));
    return final_exponentiation<Fq>(m).is_one();
}

// the device entries run on the lanes of the multi-scalar multiplication (the checks) or size fixed-base levels against free memory
// (the entries that make a key): not beside a proof that holds lanes or staging between two calls
static inline int lanes_claim(fk_ctx *ctx, const char *who) {
    if (proof_holds_lanes(ctx)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: a proof holds this context's lanes or staging buffers (collect it first: fk_prove_msms_finish_dev / fk_prove_r1cs_wait)", who);
    return scratch_claim(ctx, who);
}

static inline int draw_seed(fk_ctx *ctx, uint8_t seed[32], const char *who) {
    size_t got = 0;
    while (got < 32) {
        const ssize_t r = getrandom(seed + got, 32 - got, 0);
        if (r < 0) { if (errno == EINTR) continue; FK_SET_ERR(ctx, FK_ERR_UNSUPPORTED, "%s: getrandom failed (errno %d): no weights can be drawn", who, errno); }
        got += (size_t)r;
    }
    return FK_OK;
}

// ---- one scalar, many points (ceremony.hip: g1_scale_kernel; powers.hip: the subgroup test walks r)
// The scalar in non-adjacent form: digit i in {-1, 0, 1}, no two neighbours nonzero, at most 255 digits for k < r and a third of them
// nonzero.  `n` digits, the top one (always +1) dropped, the rest moved up so that digit n - 2 is bit 255 of its mask: the kernel walks
// the masks by shifting them left, as Xyzz::mul_affine_bits walks its scalar -- a run-time index into an array of words would put the
// array into scratch (witness.hip and poseidon.hip met that).  Passed by value: the masks live in scalar registers and every branch on a
// digit is wave-uniform.
struct NafDigits { uint64_t pos[4], neg[4]; uint32_t n; };

static NafDigits naf_recode(const Fr &k_canon) {
    uint64_t k[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) k[i] = (uint64_t)k_canon.v[2 * i] | (uint64_t)k_canon.v[2 * i + 1] << 32;
    NafDigits d;
    memset(&d, 0, sizeof d);
    uint32_t i = 0;
    while (k[0] | k[1] | k[2] | k[3] | k[4]) {
        if (k[0] & 1) {
            if ((k[0] & 3) == 1) { d.pos[i >> 6] |= (uint64_t)1 << (i & 63); k[0] -= 1; }          // (odd: no borrow)
            else { d.neg[i >> 6] |= (uint64_t)1 << (i & 63); for (int j = 0; j < 5 && ++k[j] == 0; j++) {} }
        }
        for (int j = 0; j < 4; j++) k[j] = k[j] >> 1 | k[j + 1] << 63;
        k[4] >>= 1;
        i++;
    }
    d.n = i;
    if (i == 0) return d;
    d.pos[(i - 1) >> 6] &= ~((uint64_t)1 << ((i - 1) & 63));          // the top digit is implied
    for (uint32_t s = 256 - (i - 1); s > 0; s--) {                   // (host, once per call)
        for (int j = 3; j > 0; j--) { d.pos[j] = d.pos[j] << 1 | d.pos[j - 1] >> 63; d.neg[j] = d.neg[j] << 1 | d.neg[j - 1] >> 63; }
        d.pos[0] <<= 1; d.neg[0] <<= 1;
    }
    return d;
}

// k * p for an affine p that is not the point at infinity and k.n >= 1: k.n - 1 doublings, one mixed addition of +-p per nonzero digit
template <class F>
static FK_HD Xyzz<F> mul_naf(const Affine<F> &p, NafDigits k) {
    Xyzz<F> acc{p.x, p.y, F::one(), F::one()};
    for (uint32_t left = k.n; left > 1; left--) {
        acc = Xyzz<F>::dbl(acc);
        const bool plus = k.pos[3] >> 63, minus = k.neg[3] >> 63;
        if (plus || minus) acc.add_mixed_nz(affine_neg_if(p, minus));
        for (int j = 3; j > 0; j--) { k.pos[j] = k.pos[j] << 1 | k.pos[j - 1] >> 63; k.neg[j] = k.neg[j] << 1 | k.neg[j - 1] >> 63; }
        k.pos[0] <<= 1; k.neg[0] <<= 1;
    }
    return acc;
}

// ---- a point times the lane's own scalar (ceremony_init.hip: the combinations; powers.hip: powers_scale_kernel)
// A canonical scalar as four 64-bit words, walked by shifting it left as Xyzz::mul_affine_bits walks its two: a run-time index into the
// limbs (Xyzz::mul_scalar) would put the scalar into scratch on the device.
struct K256 { uint64_t w[4]; };
static FK_HD K256 k256_of_mont(const Fr &k_mont) {
    const Fr c = Fr::from_mont(k_mont);
    K256 k;
    for (int i = 0; i < 4; i++) k.w[i] = (uint64_t)c.v[2 * i] | (uint64_t)c.v[2 * i + 1] << 32;
    return k;
}
static FK_HD void k256_shl(K256 &k) {
    k.w[3] = k.w[3] << 1 | k.w[2] >> 63; k.w[2] = k.w[2] << 1 | k.w[1] >> 63; k.w[1] = k.w[1] << 1 | k.w[0] >> 63; k.w[0] <<= 1;
}

// k * p, p affine and not the point at infinity (a term of a combination): mixed additions
template <class F>
static FK_HD Xyzz<F> mul_affine_k256(const Affine<F> &p, K256 k) {
    Xyzz<F> acc = Xyzz<F>::inf();
#pragma nounroll
    for (int i = 0; i < 256; i++) {
        acc = Xyzz<F>::dbl(acc);
        if (k.w[3] >> 63) acc.add_mixed_nz(p);
        k256_shl(k);
    }
    return acc;
}

// a host-only routine without a context leaves its message in fk_last_error(NULL)
template <class F>
static int host_entry(F &&body) {
    fk_ctx local;
    const int rc = fk_guard(&local, [&]() -> int { return body(&local); });
    try { tls_error() = local.err; } catch (...) {}
    return rc;
}

}  // namespace fk
