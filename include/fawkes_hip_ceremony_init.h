/* Key ceremony, the start of phase 2 (BGM17) in libfawkes_hip.so: derive a circuit's initial proving key from a powers-of-tau transcript
 * (phase 1) on the device, and check the transcript.  Nobody needs to know tau, alpha or beta: the derivation works on the group elements.
 *
 * The key that comes out is the Groth16 key of the circuit for the transcript's tau, alpha, beta and gamma = delta = 1 -- byte for byte what
 * fk_setup gives for those five scalars.  fk_key_contribute (fawkes_hip_ceremony.h) then takes it from there.
 *
 *   TRANSFORMS OVER GROUP ELEMENTS  fk_g1_ntt / fk_g2_ntt: out[k] = sum_j [omega^(jk)] in[j], the convention of fk_ntt (natural order in
 *       and out, omega = the 2^log_n-th root of unity of fk_ntt, the inverse uses omega^-1 and includes 1/n).
 *   THE INITIAL KEY  with rows = num_gates + num_input, m = next_pow2(rows):
 *       LG1, LA, LB (G1), LG2 (G2) = the inverse transforms of size m of the first m elements of tau_g1, alpha_tau_g1, beta_tau_g1, tau_g2
 *       h[i] = tau_g1[i + m] - tau_g1[i]  (i < m - 1)
 *       per variable v, over its columns at, bt, ct of (coeff, row) pairs (input i has one more term (1, num_gates + i) in at):
 *         a_all[v] = sum_at coeff LG1[row]   b1_all[v] = sum_bt coeff LG1[row]   b2_all[v] = sum_bt coeff LG2[row]
 *         e[v] = sum_at coeff LB[row] + sum_bt coeff LA[row] + sum_ct coeff LG1[row]
 *       ic = e of the inputs, l = e of the aux variables; a, b_g1, b_g2 = a_all, b1_all, b2_all without their points at infinity, in
 *       variable order (the only rule there is when tau is unknown; it is also the oracle's)
 *       alpha_g1 = alpha_tau_g1[0], beta_g1 = beta_tau_g1[0], beta_g2 = the transcript's; delta_g1, gamma_g2, delta_g2 = the generators
 *   THE TRANSCRIPT CHECK  fk_powers_check: with nonzero 128-bit weights rho_i (fk_ceremony_weights, fawkes_hip_ceremony.h) and, per array
 *       T of n checked elements, S = sum_{i < n - 1} rho_i T[i] and S' = sum_{i < n - 1} rho_i T[i + 1]  (n = 2m - 1 for tau_g1, m for the others)
 *         gen_ok        tau_g1[0] and tau_g2[0] are the generators
 *         tau_pair      e(tau_g1[1], G2gen) == e(G1gen, tau_g2[1])
 *         ratio_tau_g1, ratio_alpha, ratio_beta      e(S', G2gen) == e(S, tau_g2[1]) over tau_g1, alpha_tau_g1, beta_tau_g1
 *         ratio_tau_g2  e(tau_g1[1], S) == e(G1gen, S') over tau_g2
 *         beta_pair     e(beta_tau_g1[0], G2gen) == e(G1gen, beta_g2)
 *       accept = all seven.  Every flag is its predicate on its own.
 *
 * SOUNDNESS of the check.  G1 and G2 have prime order, so a ratio check passes iff sum rho_i (T[i + 1] - tau T[i]) = 0 for the tau of
 * tau_g2[1] (of tau_g1[1] for ratio_tau_g2).  For an array that is not a geometric sequence with ratio tau this is a nonzero linear form in
 * the rho_i and vanishes with probability 2^-128 over the weights.  THE STATEMENT IS VOID FOR WEIGHTS THE TRANSCRIPT'S AUTHOR CAN PREDICT:
 * pass seed = NULL (32 bytes of getrandom(2) per call) outside tests, and never a seed that was known before the transcript was published.
 * The check and the derivation ASSUME every point is on its curve and in the order-r subgroup; neither is tested here
 * (fk_points_validate and fk_powers_update_check of fawkes_hip_powers.h test both).  A key derived
 * from an inconsistent transcript is silently worthless: check first.
 *
 * Out of scope: tiled systems (copies > 1), sharded and multi-GPU keys (the key that comes out is whole, shard_count == 1), BGM17's
 * transcript hash and proofs of knowledge, the file format of any phase-1 tool (the transcript is five arrays in memory), the Rust shim.
 *
 * Points are raw affine Montgomery LE, zeros = infinity (FK_G1_BYTES / FK_G2_BYTES).  These entry points are declared here, not in
 * fawkes_hip.h (fawkes_hip_verify.h says why). */
#ifndef FAWKES_HIP_CEREMONY_INIT_H
#define FAWKES_HIP_CEREMONY_INIT_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- a powers-of-tau transcript, in memory
 * A circuit with domain m needs n_tau_g1 >= 2m - 1 and the other three counts >= m; a longer transcript is used by its prefixes, a
 * shorter one is FK_ERR_BAD_ARG with the array's name in fk_last_error. */
typedef struct {
    uint64_t n_tau_g1, n_tau_g2, n_alpha_g1, n_beta_g1;
    const uint8_t *tau_g1;        /* [tau^i] G1,        i < n_tau_g1   (64 B each) */
    const uint8_t *tau_g2;        /* [tau^i] G2,        i < n_tau_g2   (128 B each) */
    const uint8_t *alpha_tau_g1;  /* [alpha tau^i] G1,  i < n_alpha_g1 */
    const uint8_t *beta_tau_g1;   /* [beta tau^i] G1,   i < n_beta_g1 */
    const uint8_t *beta_g2;       /* [beta] G2 */
} fk_powers_desc;

/* ---- transforms over group elements, 2^log_n points, log_n = 0 .. 27 (more: FK_ERR_DOMAIN_TOO_LARGE)
 * _dev: a device array of affine points, transformed in place, asynchronous on the library's stream.  The work array (128 B per point in
 * G1, 256 B in G2) is a buffer of the context that fk_trim releases; the twiddles are the tables of fk_ntt's domain of the same size.
 * fk_g1_ntt / fk_g2_ntt: host arrays, out may be the input.  With ctx == NULL they are plain host C++ (the reference the kernels are
 * compared with, one generic double-and-add per butterfly), with a context the points go through the kernels.
 * [staging] with a context they borrow the staging buffers. */
int fk_g1_ntt_dev(fk_ctx *ctx, void *d_points, uint32_t log_n, int inverse);
int fk_g2_ntt_dev(fk_ctx *ctx, void *d_points, uint32_t log_n, int inverse);
int fk_g1_ntt(fk_ctx *ctx, const uint8_t *points, uint32_t log_n, int inverse, uint8_t *out);
int fk_g2_ntt(fk_ctx *ctx, const uint8_t *points, uint32_t log_n, int inverse, uint8_t *out);

/* ---- the initial key
 * A NEW whole resident key on ctx's device, laid out as fk_setup's (shard_count == 1); vk_out and ic_out as fk_setup's: alpha_g1, beta_g1,
 * beta_g2, gamma_g2, delta_g1, delta_g2 in slots of 128 bytes, and num_input points.  flags: FK_KEY_NO_LEVELS or 0 (otherwise the
 * fixed-base levels are derived at the end, as by fk_setup).  m >= 2^28 is FK_ERR_DOMAIN_TOO_LARGE; num_input == 0, a variable index out
 * of range, a null pointer or a transcript that is too short FK_ERR_BAD_ARG.  Blocks until the key is complete; every temporary is
 * released before the levels are sized (the transform's tables stay with the context's domain, as after fk_ntt).
 * Refused (FK_ERR_BAD_ARG) while a proof holds the context's lanes or staging (fk_prove_msms_z_begin_dev, fk_prove_r1cs_submit). */
int fk_key_from_powers(fk_ctx *ctx, const fk_powers_desc *p, const fk_r1cs *cs, uint32_t flags, fk_key **out_key, uint8_t vk_out[6 * 128], uint8_t *ic_out);
/* The reference (no GPU, plain loops; about 0.2 ms per point multiplication in G1 and three times that in G2: domains up to 2^8 or so).
 * h_out: m - 1 points; l_out: num_aux; a_out, b_g1_out (64 B each) and b_g2_out (128 B each): room for num_input + num_aux points, of
 * which counts_out[0] (a) and counts_out[1] (b_g1, b_g2) are written; vk_out, ic_out as above. */
int fk_key_from_powers_host(const fk_powers_desc *p, const fk_r1cs *cs, uint8_t *h_out, uint8_t *l_out, uint8_t *a_out, uint8_t *b_g1_out,
                            uint8_t *b_g2_out, uint64_t counts_out[2], uint8_t vk_out[6 * 128], uint8_t *ic_out);

/* ---- the transcript check, over the prefixes a circuit with domain m uses (m >= 2; not necessarily a power of two) */
typedef struct {
    int32_t accept;            /* all seven below */
    int32_t gen_ok, tau_pair, ratio_tau_g1, ratio_tau_g2, ratio_alpha, ratio_beta, beta_pair;
    uint8_t s_tau_g1[64], s_tau_g1_next[64], s_alpha[64], s_alpha_next[64], s_beta[64], s_beta_next[64];      /* S and S', raw affine */
    uint8_t s_tau_g2[128], s_tau_g2_next[128];
    uint8_t seed[32];          /* the seed the weights came from: the same call with this seed reproduces the report */
} fk_powers_report;

/* A failed check is accept = 0 with FK_OK; only malformed arguments fail the call (null pointers, m < 2, a transcript that is too short:
 * FK_ERR_BAD_ARG).  seed == NULL: 32 bytes of getrandom(2), FK_ERR_UNSUPPORTED if that fails.
 * fk_powers_check: the arrays are staged on the device, the 2m - 2 weights generated there once, the eight sums run through the
 * multi-scalar multiplication over an array and the same array one element on, the pairings run on the host.  Blocks until the verdict is
 * known.  [staging]; refused while a proof holds the context's lanes or staging, like fk_key_from_powers.
 * fk_powers_check_host: the reference (no GPU): naive sums, the same pairings; seed must be given. */
int fk_powers_check(fk_ctx *ctx, const fk_powers_desc *p, uint64_t m, const uint8_t *seed, fk_powers_report *report);
int fk_powers_check_host(const fk_powers_desc *p, uint64_t m, const uint8_t seed[32], fk_powers_report *report);

#ifdef __cplusplus
}
#endif
#endif
