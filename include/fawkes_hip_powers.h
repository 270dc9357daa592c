/* Key ceremony, phase 1 (BGM17) in libfawkes_hip.so: contribute to a powers-of-tau transcript on the device, validate the points of one
 * that somebody else hands over, and check that one transcript is another with exactly one contribution applied.
 *
 * A transcript (fk_powers_desc, fawkes_hip_ceremony_init.h) holds [tau^i] G1, [tau^i] G2, [alpha tau^i] G1, [beta tau^i] G1 and [beta] G2.
 *
 *   A POINT TIMES ITS OWN POWER  fk_g1_scale_powers / fk_g2_scale_powers: out[i] = [c x^(first + i) mod r] in[i].
 *   CONTRIBUTE with secrets x, y, z (all nonzero):
 *       tau_g1'[i] = [x^i] tau_g1[i]                tau_g2'[i] = [x^i] tau_g2[i]
 *       alpha_tau_g1'[i] = [y x^i] alpha_tau_g1[i]  beta_tau_g1'[i] = [z x^i] beta_tau_g1[i]      beta_g2' = [z] beta_g2
 *       i.e. tau' = x tau, alpha' = y alpha, beta' = z beta; and the public part of the contribution, pub = [x] G2gen, [y] G2gen, [z] G2gen.
 *       fk_powers_new gives the transcript of tau = alpha = beta = 1 (the generators): a transcript from known secrets is
 *       contribute(new(m), tau, alpha, beta).
 *   VALIDATE POINTS  fk_points_validate: every point falls in exactly one class, tested in this order:
 *         infinity   the point is all zeros (a transcript holds no point at infinity: every secret is nonzero)
 *         range      some coordinate's limbs are not below q
 *         curve      y^2 != x^3 + b (G1), y^2 != x^3 + b' over Fq2 (G2)
 *         subgroup   G2 only (G1 has cofactor 1): [r] P is not the point at infinity
 *       and is good otherwise.  The report holds the four counts and first_bad, the lowest index in any of the four classes.
 *   CHECK AN UPDATE  fk_powers_update_check: `after` against `before` and pub, without any secret, over the prefixes a domain of m uses
 *         shape_ok     both transcripts are long enough for m (2m - 1 of tau_g1, m of the others)
 *         points_ok    no point of `after` is in any of the four classes above (beta_g2 counts as an array of one)
 *         after        the whole report of fk_powers_check on `after`: seven flags, eight sums, the seed
 *         step_tau     e(after.tau_g1[1], G2gen) == e(before.tau_g1[1], pub.x_g2)
 *         step_alpha   e(after.alpha_tau_g1[0], G2gen) == e(before.alpha_tau_g1[0], pub.y_g2)
 *         step_beta    e(after.beta_tau_g1[0], G2gen) == e(before.beta_tau_g1[0], pub.z_g2)
 *         changed      informational: after.tau_g1[1] != before.tau_g1[1] (x = 1 is a valid contribution)
 *       accept = shape_ok, points_ok, after.accept and the three steps.  Every flag is its predicate on its own, with two exceptions that
 *       keep every verdict a statement about group elements: with shape_ok = 0 nothing else is looked at (all other fields are zero, the
 *       reports' first_bad UINT64_MAX); and a point with a range or curve failure is never paired -- a pairing flag (of `after` or a step)
 *       that reads such a single point (of `after`, `before` or pub) is 0, and an array of `after` with such a point is not summed: its
 *       ratio flag is 0 and its two sums are zeros.  Points outside the subgroup are on the curve and are summed and paired as they are.
 *
 * SOUNDNESS of the update check.  fk_powers_check's statement (fawkes_hip_ceremony_init.h) makes `after` a transcript of SOME tau',
 * alpha', beta': its ratio statements are VOID FOR WEIGHTS THE TRANSCRIPT'S AUTHOR CAN PREDICT -- pass seed = NULL (32 bytes of getrandom(2)
 * per call) outside tests, and never a seed that was known before `after` was published.  That statement assumes points on their curves
 * and in the order-r subgroup, which points_ok establishes for `after`; `before` is assumed to have been accepted earlier.  The step
 * equations bind `after` to `before` through pub: with the x of pub.x_g2 = [x] G2gen, step_tau holds iff tau' = x tau, likewise alpha' =
 * y alpha and beta' = z beta (beta_g2' is tied to beta_tau_g1'[0] by fk_powers_check's beta_pair).  Nothing here shows that the contributor
 * KNEW x, y, z.
 *
 * Out of scope: BGM17's proofs of knowledge and transcript hash (host work on a few points; pub and the report carry what they need), the
 * .ptau format and any other file format (a transcript is five arrays in memory), multi-GPU, the Rust shim.
 *
 * Scalars (x, y, z, c) are Montgomery Fr limbs, the form fk_key_contribute takes its x; zero or an image >= r is FK_ERR_BAD_ARG.  Points
 * are raw affine Montgomery LE, zeros = infinity (FK_G1_BYTES / FK_G2_BYTES).  A host entry without a context is the plain-loop reference
 * the device is compared with (about 0.2 ms per multiplication in G1 and three times that in G2).  _dev entries are asynchronous on the
 * library's stream.  [staging] entries borrow the staging buffers and are refused (FK_ERR_BAD_ARG) while a proof holds the context's lanes
 * or staging (fk_prove_msms_z_begin_dev, fk_prove_r1cs_submit).  These entry points are declared here, not in fawkes_hip.h
 * (fawkes_hip_verify.h says why). */
#ifndef FAWKES_HIP_POWERS_H
#define FAWKES_HIP_POWERS_H
#include "fawkes_hip_ceremony_init.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- a point times its own power of x
 * out[i] = [c x^(first + i) mod r] in[i] for i < n, affine; the point at infinity stays the point at infinity.  `first` lets a long array
 * be done in pieces (first + n must not pass 2^64).  _dev: device pointers; d_out == d_in is allowed (otherwise the two must not overlap);
 * n == 0 writes nothing.  fk_g1_scale_powers / fk_g2_scale_powers: host buffers, out may be the input; with ctx == NULL plain host C++ over
 * the generic double-and-add, with a context the points go through the kernel.  [staging] with a context. */
int fk_g1_scale_powers_dev(fk_ctx *ctx, const void *d_in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], void *d_out);
int fk_g2_scale_powers_dev(fk_ctx *ctx, const void *d_in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], void *d_out);
int fk_g1_scale_powers(fk_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], uint8_t *out);
int fk_g2_scale_powers(fk_ctx *ctx, const uint8_t *in, uint64_t n, uint64_t first, const uint64_t x[4], const uint64_t c[4], uint8_t *out);

/* ---- contribute */
typedef struct {                  /* five caller-owned host arrays, with the counts of the transcript they are made from */
    uint8_t *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1;
    uint8_t *beta_g2;             /* 128 bytes */
} fk_powers_out;
typedef struct { uint8_t x_g2[128], y_g2[128], z_g2[128]; } fk_powers_public;      /* [x] G2gen, [y] G2gen, [z] G2gen */

/* The transcript of tau = alpha = beta = 1 for a domain of m >= 1: 2m - 1 generators in tau_g1, m in each of the other three, the G2
 * generator in beta_g2.  Host only. */
int fk_powers_new(uint64_t m, fk_powers_out *out);
/* `in` is only read, whole (every element of every array, whatever domain it was made for); tau_g1 must hold at least two elements and
 * the others one (less cannot be bound by an update check: FK_ERR_BAD_ARG).  fk_powers_contribute: the four arrays are staged and scaled
 * one after another (the peak of device memory is one array), the single points (beta_g2' and pub) are computed on the host while the
 * first kernel runs.  Blocks until `out` is complete.  [staging].  fk_powers_contribute_host: the reference (no GPU). */
int fk_powers_contribute(fk_ctx *ctx, const fk_powers_desc *in, const uint64_t x[4], const uint64_t y[4], const uint64_t z[4], fk_powers_out *out, fk_powers_public *pub);
int fk_powers_contribute_host(const fk_powers_desc *in, const uint64_t x[4], const uint64_t y[4], const uint64_t z[4], fk_powers_out *out, fk_powers_public *pub);

/* ---- validate points */
typedef struct {
    uint64_t infinity, range, curve, subgroup;      /* points per class */
    uint64_t first_bad;                             /* the lowest index in any of the four classes, UINT64_MAX if there is none */
} fk_points_report;

/* n points of G1 (g2 == 0, 64 bytes each) or G2 (g2 == 1, 128 bytes each; any other value: FK_ERR_BAD_ARG).  fk_points_validate: host
 * points; with ctx == NULL the reference, with a context through the kernel ([staging], blocks).  fk_points_validate_dev: the points AND
 * the report (sizeof(fk_points_report) bytes, 8-byte aligned) in device memory, asynchronous.  Bad coordinates are only arithmetic. */
int fk_points_validate(fk_ctx *ctx, const uint8_t *pts, uint64_t n, int g2, fk_points_report *rep);
int fk_points_validate_dev(fk_ctx *ctx, const void *d_pts, uint64_t n, int g2, void *d_rep);

/* ---- check an update */
typedef struct {
    int32_t accept;               /* shape_ok, points_ok, after.accept, step_tau, step_alpha, step_beta */
    int32_t shape_ok, points_ok, step_tau, step_alpha, step_beta;
    int32_t changed;              /* informational */
    int32_t reserved;
    fk_points_report tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2;      /* the points of `after`, over the checked prefixes */
    fk_powers_report after;
} fk_powers_update_report;

/* A failed check is accept = 0 with FK_OK; only malformed arguments fail the call (null pointers or arrays, m < 2 or m >= 2^28, arrays of
 * `after` that are not 16-byte aligned: FK_ERR_BAD_ARG).  seed == NULL: 32 bytes of getrandom(2), FK_ERR_UNSUPPORTED if that fails.
 * fk_powers_update_check: the arrays of `after` are staged and validated one after another, then checked by fk_powers_check; the pairings
 * run on the host.  Blocks until the verdict is known.  [staging].
 * fk_powers_update_check_host: the reference (no GPU); seed must be given. */
int fk_powers_update_check(fk_ctx *ctx, const fk_powers_desc *before, const fk_powers_desc *after, const fk_powers_public *pub, uint64_t m,
                           const uint8_t *seed, fk_powers_update_report *rep);
int fk_powers_update_check_host(const fk_powers_desc *before, const fk_powers_desc *after, const fk_powers_public *pub, uint64_t m,
                                const uint8_t seed[32], fk_powers_update_report *rep);

#ifdef __cplusplus
}
#endif
#endif
