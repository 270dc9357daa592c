// What ceremony.hip (one phase-2 step) and ceremony_init.hip (the initial key from a powers-of-tau transcript) both use on the host: the
// generators, the pairing comparison of a check, the seed of its weights, the claim of a device entry and the frame of a host-only entry.
#pragma once
#include "common.hpp"
#include "pairing.hpp"
#include <sys/random.h>
#include <errno.h>

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

// a host-only routine without a context leaves its message in fk_last_error(NULL)
template <class F>
static int host_entry(F &&body) {
    fk_ctx local;
    const int rc = fk_guard(&local, [&]() -> int { return body(&local); });
    try { tls_error() = local.err; } catch (...) {}
    return rc;
}

}  // namespace fk
