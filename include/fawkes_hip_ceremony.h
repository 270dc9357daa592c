/* Key ceremony (phase 2, BGM17) of libfawkes_hip.so: apply one delta contribution to a proving key, and check one, on the device.
 *
 * A key holds delta_g1, delta_g2, h[i] = [tau^i t(tau) / delta] G1 (i < n_h), l[k] = [(beta A_k + alpha B_k + C_k) / delta] G1 (aux
 * variables), and parts that do not depend on delta: alpha_g1, beta_g1, beta_g2, a, b_g1, b_g2 (gamma_g2 and ic belong to the verifying
 * key and travel beside the proving key, as everywhere in fawkes_hip.h).
 *
 *   CONTRIBUTE with x != 0:  delta_g1' = [x] delta_g1, delta_g2' = [x] delta_g2, h'[i] = [1/x] h[i], l'[k] = [1/x] l[k]; everything
 *       else is copied.  The point at infinity stays the point at infinity (l holds it for a variable that occurs in no constraint).
 *   CHECK `after` against `before` without knowing x, with nonzero 128-bit weights rho_i (fk_ceremony_weights) drawn AFTER `after` is fixed:
 *       S_h = sum rho_i h[i], S_h' = sum rho_i h'[i], likewise S_l, S_l'.  Accept iff
 *         shape_equal    m, num_input, num_aux, n_h, n_l, n_a, n_b are equal
 *         fixed_equal    alpha_g1, beta_g1, beta_g2 and the arrays a, b_g1, b_g2 are equal byte for byte
 *         delta_nonzero  neither new delta is the point at infinity
 *         delta_pair     e(delta_g1', G2gen) == e(G1gen, delta_g2')
 *         ratio_h        e(S_h', delta_g2') == e(S_h, delta_g2)
 *         ratio_l        e(S_l', delta_g2') == e(S_l, delta_g2)
 *       Every flag is its predicate on its own; with unequal shapes the arrays cannot be paired up, so fixed_equal, ratio_h and ratio_l are
 *       then 0 and the four sums are zeros.  delta_changed (delta_g1' != delta_g1) is informational: x = 1 is a valid contribution.
 *
 * SOUNDNESS.  G1 has prime order and delta_g2 != 0, so a ratio check passes iff sum rho_i (x h'[i] - h[i]) = 0 for the x with
 * delta_g2' = [x] delta_g2.  For any h' that is not [1/x] h this is a nonzero linear form in the rho_i; it vanishes with probability
 * 2^-128 over the weights.  THE STATEMENT IS VOID FOR WEIGHTS THE CONTRIBUTOR CAN PREDICT: pass seed = NULL (32 bytes of getrandom(2) per
 * call) outside tests, and never a seed that was known before `after` was published.  The check ASSUMES every point is on its curve and
 * in the order-r subgroup: that is the loader's job (fk_key_load_bellman with FK_KEY_CHECKED), not repeated here.
 *
 * Out of scope: BGM17's proof of knowledge of x and the transcript hash (host work on three points and a hash-to-G2: the report and the
 * returned deltas carry what it needs), phase 1, sharded and multi-GPU keys (shard_count != 1: FK_ERR_BAD_ARG), the Rust shim.
 *
 * Scalars (k, x) are Montgomery Fr limbs like r and s of fk_prove; an image >= r is FK_ERR_FORMAT.  Points are raw affine Montgomery LE,
 * zeros = infinity (FK_G1_BYTES / FK_G2_BYTES).  These entry points are declared here, not in fawkes_hip.h (fawkes_hip_verify.h says why). */
#ifndef FAWKES_HIP_CEREMONY_H
#define FAWKES_HIP_CEREMONY_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- many points times ONE scalar
 * out[i] = k * in[i], affine.  _dev: device pointers, asynchronous on the library's stream; d_out == d_in is allowed (otherwise the two must
 * not overlap); n == 0 writes nothing.  fk_g1_scale: host buffers; with ctx == NULL it is plain host C++ over the generic double-and-add
 * (the reference the kernel is compared with, ~0.17 ms per point on one core), with a context the points go through the kernel.
 * [staging] fk_g1_scale with a context borrows the staging buffers. */
int fk_g1_scale_dev(fk_ctx *ctx, const void *d_in, size_t n, const uint64_t k[4], void *d_out);
int fk_g1_scale(fk_ctx *ctx, const uint8_t *in, size_t n, const uint64_t k[4], uint8_t *out);

/* ---- contribute
 * A NEW resident key on ctx's device from `key` (whole, on the same device) and x != 0 (x == 0: FK_ERR_BAD_ARG).  a, b_g1, b_g2 are
 * copied device to device, h and l go through the scale kernel with 1/x, the two deltas are scaled with x on the host.  `key` is only
 * read: contexts that are proving from it are not disturbed.  flags: FK_KEY_NO_LEVELS or 0 (otherwise the fixed-base levels are derived
 * at the end, as by fk_setup).  fk_key_vk(*out_key) gives the new deltas for the verifying key.
 * Refused (FK_ERR_BAD_ARG) while a proof holds the context's lanes or staging (fk_prove_msms_z_begin_dev, fk_prove_r1cs_submit). */
int fk_key_contribute(fk_ctx *ctx, const fk_key *key, const uint64_t x[4], uint32_t flags, fk_key **out_key);
/* The reference over a host key description (no GPU): h_out (n_h x 64), l_out (n_l x 64), delta_g1_out (64), delta_g2_out (128). */
int fk_key_contribute_host(const fk_key_desc *in, const uint64_t x[4], uint8_t *h_out, uint8_t *l_out, uint8_t *delta_g1_out, uint8_t *delta_g2_out);

/* ---- the weights of a check
 * n Montgomery Fr images, 32 bytes each (the scalar form of fk_msm_g1*).  Weight i is the little-endian 128-bit integer in words
 * 4 (i mod 4) .. 4 (i mod 4) + 3 of block i / 4 of the ChaCha20 stream with key = seed (eight LE words), 64-bit block counter, stream id 0;
 * a zero draw becomes 1.  The bytes are the specification: host and device agree exactly.  _dev: asynchronous on the library's stream. */
int fk_ceremony_weights(const uint8_t seed[32], size_t n, uint64_t *out);
int fk_ceremony_weights_dev(fk_ctx *ctx, const uint8_t seed[32], size_t n, void *d_out);

/* ---- check */
typedef struct {
    int32_t accept;            /* all six below */
    int32_t shape_equal, fixed_equal, delta_nonzero, delta_pair, ratio_h, ratio_l;
    int32_t delta_changed;     /* informational */
    uint8_t s_h[64], s_h_after[64], s_l[64], s_l_after[64];      /* the four sums, raw affine */
    uint8_t seed[32];          /* the seed the weights came from: the same call with this seed reproduces the report */
} fk_contribution_report;

/* A failed check is accept = 0 with FK_OK; only malformed arguments fail the call (null pointers, a sharded key, keys that are not on
 * ctx's device: FK_ERR_BAD_ARG).  seed == NULL: 32 bytes of getrandom(2), FK_ERR_UNSUPPORTED if that fails.
 * fk_key_contribution_check: resident keys.  The weights are generated once (max(n_h, n_l) of them, in a buffer of the context that
 * fk_trim releases), the four sums run through the multi-scalar multiplication over the keys' own h and l, a, b_g1 and b_g2 are compared
 * on the device, the pairings run on the host.  Blocks until the verdict is known.  Refused while a proof holds the context's lanes or
 * staging, like fk_key_contribute.
 * fk_key_contribution_check_host: the reference over two host descriptions (no GPU): naive sums, the same pairings; seed must be given. */
int fk_key_contribution_check(fk_ctx *ctx, const fk_key *before, const fk_key *after, const uint8_t *seed, fk_contribution_report *report);
int fk_key_contribution_check_host(const fk_key_desc *before, const fk_key_desc *after, const uint8_t seed[32], fk_contribution_report *report);

#ifdef __cplusplus
}
#endif
#endif
