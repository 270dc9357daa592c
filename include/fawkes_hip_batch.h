/* Batch prover of libfawkes_hip.so: `count` Groth16 proofs of ONE small circuit under ONE key in one call.
 *
 * fk_prove_r1cs_dev proves one large system at a time; its schedules (sorts first, early front, lanes, fixed-base levels) are tuned for
 * 2^22 .. 2^27 rows.  A relayer proving tree updates or a service proving client transfers has the opposite shape: thousands of proofs
 * of a circuit of a few thousand gates, all against one key.  The entry points below run every stage of such proofs with the proof
 * index as a second grid dimension: per GROUP of proofs the number of kernel launches is fixed (fk_batch_plan_info.launches_per_group)
 * and the host blocks once, at the download of the group's proofs.
 *
 * Proof i is byte for byte what fk_prove_r1cs_dev(key, r1cs, z_i, r_i, s_i) returns: the 256 bytes are a function of (key, witness, r, s)
 * only, because the points are normalised to affine (csrc/batch_prove.hip).
 *
 * Declared here and not in fawkes_hip.h for the reason given in fawkes_hip_witness.h: that header is one pinned ABI. */
#ifndef FAWKES_HIP_BATCH_H
#define FAWKES_HIP_BATCH_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* where variable v of proof i lives in the witness array */
#define FK_BATCH_Z_ROWS 0  /* count rows of num_input + num_aux elements, each row with its own ONE at [0] */
#define FK_BATCH_Z_TILED 1 /* fk_r1cs_load_tiled / fk_witness_generate_dev order for `count` copies:
                              ONE, copy 0's inputs, copy 1's inputs, ..., copy 0's aux, copy 1's aux, ... */

#define FK_BATCH_MAX_LOG_M 20       /* above 2^20 rows one proof fills the device: fk_prove_r1cs_dev */
#define FK_BATCH_WINDOW_BITS_MIN 2  /* the bucket kernels' compiled limits for a forced window width */
#define FK_BATCH_WINDOW_BITS_MAX 14
#define FK_BATCH_MAX_GROUP 32768    /* proofs per group (the proof index is a grid dimension) */
/* scratch budget when fk_batch_opts.scratch_budget_bytes is 0: fk_prove_batch_dev and the stage entries take a quarter of the HBM that is
 * free when they are called (plus what the batch scratch already holds); fk_prove_batch_plan, which sees no GPU, assumes this much */
#define FK_BATCH_PLAN_DEFAULT_BUDGET (16ull << 30)
#define FK_BATCH_BUDGET_FREE_DIVISOR 4

typedef struct {
    uint64_t scratch_budget_bytes;                 /* 0 = the default above */
    uint32_t window_bits_g1, window_bits_g2;       /* 0 = the plan's choice, else FK_BATCH_WINDOW_BITS_MIN .. _MAX */
} fk_batch_opts;

typedef struct {
    uint32_t group, n_groups;                      /* proofs per group (the last group may hold fewer), groups */
    uint32_t window_bits_g1, windows_g1;           /* signed-digit windows: windows * bits >= 255 */
    uint32_t window_bits_g2, windows_g2;
    uint32_t segment;                              /* entries of a bucket one lane accumulates */
    uint32_t ntt_passes;                           /* passes of one transform of the domain */
    uint32_t launches_per_group;                   /* kernels, memsets and device scans queued per group: independent of count */
    uint32_t reserved;
    uint64_t scratch_bytes;                        /* device scratch of one group */
} fk_batch_plan_info;

typedef struct { double eval_ms, quotient_ms, msm_h_ms, msm_l_ms, msm_a_ms, msm_b1_ms, msm_b2_ms, assemble_ms, total_ms; } fk_batch_timings;

/* Host only, no GPU.  m: the key's domain (a power of two, 2 .. 2^20); n_l, n_a, n_b: the key's query lengths (the H query has m - 1).
 * FK_ERR_BAD_ARG (message in fk_last_error(NULL)) for m not a power of two, m < 2, m > 2^20, forced window bits out of range, out == NULL.
 * The group is the largest one whose scratch fits the budget; a group of 1 is always allowed. */
int fk_prove_batch_plan(uint64_t m, uint64_t n_l, uint64_t n_a, uint64_t n_b, uint32_t count, const fk_batch_opts *opts, fk_batch_plan_info *out);

/* d_z: the witnesses on the device in `z_layout`; r, s: count x 4 Montgomery limbs (host); out_proofs: count x 256 bytes (host).
 * opts, tm may be NULL.  count == 0: FK_OK, nothing written.  Refusals (nothing is dropped, the context stays usable):
 *   FK_ERR_BAD_ARG       a tiled system (copies > 1), a sharded key, m > 2^20 (use fk_prove_r1cs_dev), a null pointer, an unknown layout
 *   FK_ERR_KEY_MISMATCH  where fk_prove_r1cs_dev gives it (variable counts, rows against the domain, query lengths)
 *   FK_ERR_UNEXPECTED_IDENTITY  delta is the identity
 *   [staging] FK_ERR_BAD_ARG while a submitted proof (fk_prove_r1cs_submit) or any witness multiplication is outstanding
 * The batch scratch is the context's own (released by fk_trim / fk_free) and aliases neither the lanes' nor the staging scratch. */
int fk_prove_batch_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const void *d_z, int z_layout, uint32_t count,
                       const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm);
/* the same with the witnesses on the host, as FK_BATCH_Z_ROWS rows */
/* [staging] */
int fk_prove_batch(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const uint64_t *z, uint32_t count,
                   const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm);

/* ---- the stages alone (micro entry points in the sense of fk_msm_g1_dev / fk_quotient_h_dev); device pointers, one group, blocking */
/* d_a, d_b, d_c: count x m elements each, m = next_pow2(num_gates + num_input); row t of proof i at [i * m + t], zero behind the rows */
int fk_batch_r1cs_eval_dev(fk_ctx *ctx, const fk_r1cs_dev *r1cs, const void *d_z, int z_layout, uint32_t count, void *d_a, void *d_b, void *d_c);
/* d_a, d_b, d_c: count x 2^log_m, the first n_rows of each row valid (the rest is zeroed here); all three are used as scratch.
 * d_h: count x 2^log_m, the first 2^log_m - 1 of each row are the quotient's coefficients */
int fk_batch_quotient_dev(fk_ctx *ctx, void *d_a, void *d_b, void *d_c, uint64_t n_rows, uint32_t log_m, uint32_t count, void *d_h);
/* out[i] = sum_j scalar(i, j) * bases[j], j < n, raw affine (64 B, or 128 B with g2 != 0; zeros = infinity).
 * scalar(i, j) = variable (d_idx ? d_idx[j] : var_offset + j) of proof i's witness in d_z; the witness has z_vars variables of which the first
 * num_input are the inputs (FK_BATCH_Z_ROWS ignores num_input and takes z_vars as the row length). */
int fk_batch_msm_dev(fk_ctx *ctx, const void *d_bases, uint64_t n, int g2, const uint32_t *d_idx, uint32_t var_offset, const void *d_z,
                     int z_layout, uint32_t num_input, uint32_t z_vars, uint32_t count, const fk_batch_opts *opts, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
