// What the two verifier translation units share (verify.hip: one equation per proof; verify_agg.hip: one aggregated equation per
// batch): the Borsh decoders of a coordinate and a point, and the check of a verifying key's framing against the input count.
#pragma once
#include "common.hpp"
#include "pairing.hpp"
#include <string.h>

namespace fk {

template <class Fq>
static FK_HD Fq canon_to_mont(const uint8_t *p, bool *ok) {
    Fq v;
    for (int i = 0; i < 8; i++) v.v[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    bool below = false;
    for (int i = 7; i >= 0; i--) {
        if (v.v[i] < FqParams::p(i)) { below = true; break; }
        if (v.v[i] > FqParams::p(i)) break;
    }
    if (!below) *ok = false;                       // Num<Fq>::deserialize: from_uint fails for values >= q
    return Fq::to_mont(v);
}
template <class Fq>
static FK_HD Affine<Fq> g1_from_borsh(const uint8_t *p, bool *ok) { return Affine<Fq>{canon_to_mont<Fq>(p, ok), canon_to_mont<Fq>(p + 32, ok)}; }
template <class Fq>
static FK_HD Affine<Fq2T<Fq>> g2_from_borsh(const uint8_t *p, bool *ok) {
    Affine<Fq2T<Fq>> a;
    a.x.c0 = canon_to_mont<Fq>(p, ok); a.x.c1 = canon_to_mont<Fq>(p + 32, ok);
    a.y.c0 = canon_to_mont<Fq>(p + 64, ok); a.y.c1 = canon_to_mont<Fq>(p + 96, ok);
    return a;
}

static inline int vk_check(fk_ctx *ctx, const uint8_t *vk, size_t vk_len, uint32_t n_inputs, uint32_t *n_ic) {
    if (!vk || vk_len < 456) FK_SET_ERR(ctx, FK_ERR_FORMAT, "verify: verifying key truncated");
    uint32_t n; memcpy(&n, vk + 448, 4);
    if (vk_len != 452 + (size_t)n * 64) FK_SET_ERR(ctx, FK_ERR_FORMAT, "verify: verifying key holds %u ic points but is %zu bytes long", n, vk_len);
    // bellman verify_proof: (public_inputs.len() + 1) != pvk.ic.len() -> SynthesisError::MalformedVerifyingKey
    if (n != n_inputs + 1) FK_SET_ERR(ctx, FK_ERR_KEY_MISMATCH, "verify: %u public inputs for a key with %u ic points", n_inputs, n);
    *n_ic = n;
    return FK_OK;
}

}  // namespace fk
