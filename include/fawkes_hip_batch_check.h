/* The batch prover's R1CS check of libfawkes_hip.so: one verdict per proof of a batch, from the evaluation the proofs are made from.
 *
 * fk_prove_batch_dev hands back 256 well-formed bytes for a bad signature or a stale Merkle path exactly as for a good witness (the
 * prover's bytes are defined for any witness).  The entry points below say WHICH proofs of a batch are worthless, and which gates of
 * them are violated: what fk_r1cs_check_dev / fk_prove_r1cs_checked_dev (fawkes_hip_check.h) say of one large system, said of every
 * proof of a batch, with the proof index as a second grid dimension (csrc/batch_check.hip, DESIGN.md sections 3.9 and 3.10).
 *
 * One fk_check_report per proof:
 *   gates                   num_gates of the instance
 *   n_groups, n_bad_groups  0, 0
 *   n_bad, first_bad, first_abc   over that proof's own gates; first_bad is a gate index within the instance
 *   n_range, first_range    over that proof's own num_input + num_aux variables; first_range is the variable index in the instance's
 *                           numbering, not a place in the witness array
 *   one_ok                  FK_BATCH_Z_ROWS: the proof's own z[0].  FK_BATCH_Z_TILED: the one shared ONE -- the same in every report,
 *                           and a shared ONE that is not below r counts in every proof's n_range
 *   gates_valid             0 for a proof with n_range > 0: its gates are then not judged (n_bad = 0, first_bad = FK_CHECK_NONE, its
 *                           bitmap words zero); every other proof's report stays exact
 * Optional outputs, either may be NULL, nothing outside these extents is written:
 *   bad_bitmap   count x ceil(gates / 64) words, proof-major: bit g % 64 of word g / 64 of proof i set iff gate g of proof i is bad.
 *                Every word is written (the caller does not zero it); the bits at and beyond `gates` are zero.
 *   proof_bad    count bytes: byte i is 1 iff n_bad > 0 || n_range > 0 || !one_ok of proof i.
 * A violated witness is NOT an error: the calls return FK_OK and the reports speak.  count == 0: FK_OK, nothing written.
 *
 * Declared here and not in fawkes_hip.h for the reason given in fawkes_hip_witness.h: that header is one pinned ABI. */
#ifndef FAWKES_HIP_BATCH_CHECK_H
#define FAWKES_HIP_BATCH_CHECK_H
#include "fawkes_hip_batch.h"
#include "fawkes_hip_check.h"
#ifdef __cplusplus
extern "C" {
#endif

/* kernels the check adds to a group of proofs, whatever count is: the records, the range, the gates, the closing
 * (fk_batch_plan_info.launches_per_group keeps describing the unchecked call) */
#define FK_BATCH_CHECK_LAUNCHES 4
/* device scratch of the check per proof of a group (one record), on top of the three rows of the evaluation */
#define FK_BATCH_CHECK_RECORD_BYTES 160

/* host, ctx may be NULL, no GPU: the reference the device entries are compared with.  cs = ONE instance; z = the witnesses of `count`
 * proofs in z_layout; bad_bitmap, proof_bad and reports are host arrays.  FK_ERR_BAD_ARG for a null system, witness or reports, an
 * unknown layout and a system without the input ONE. */
int fk_batch_r1cs_check(fk_ctx *ctx, const fk_r1cs *cs, const uint64_t *z, int z_layout, uint32_t count,
                        uint64_t *bad_bitmap, uint8_t *proof_bad, fk_check_report *reports);

/* device: evaluates and checks, with no key and no proof.  d_z as for fk_prove_batch_dev; d_bad_bitmap / d_proof_bad are device
 * pointers; reports is a host pointer.  Any count: the call works in groups of g proofs, the largest g (at most FK_BATCH_MAX_GROUP) with
 * g * (3 * m * 32 + FK_BATCH_CHECK_RECORD_BYTES) <= the budget of opts (fk_batch_opts.scratch_budget_bytes; the window widths are not
 * used), m = next_pow2(num_gates + num_input), and at least 1; it blocks once per group.
 * Refusals are those of fk_batch_r1cs_eval_dev, plus FK_ERR_BAD_ARG for reports == NULL. */
/* [staging] */
int fk_batch_r1cs_check_dev(fk_ctx *ctx, const fk_r1cs_dev *r1cs, const void *d_z, int z_layout, uint32_t count,
                            void *d_bad_bitmap, void *d_proof_bad, fk_check_report *reports, const fk_batch_opts *opts);

/* fk_prove_batch_dev plus the check of the SAME evaluation: the check is queued between the evaluation and the quotient of each group,
 * and the group's reports come down with the group's proofs -- still one host block per group.  out_proofs holds the bytes of
 * fk_prove_batch_dev whether or not a witness satisfies the system.  tm is filled as fk_prove_batch_dev fills it; the check's device
 * time goes to *check_ms alone (may be NULL) and into no stage of tm.  Refusals are those of fk_prove_batch_dev, plus FK_ERR_BAD_ARG
 * for reports == NULL. */
int fk_prove_batch_checked_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const void *d_z, int z_layout, uint32_t count,
                               const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm,
                               void *d_bad_bitmap, void *d_proof_bad, fk_check_report *reports, double *check_ms);
/* the same with the witnesses on the host, as FK_BATCH_Z_ROWS rows */
/* [staging] */
int fk_prove_batch_checked(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const uint64_t *z, uint32_t count,
                           const uint64_t *r, const uint64_t *s, uint8_t *out_proofs, const fk_batch_opts *opts, fk_batch_timings *tm,
                           void *d_bad_bitmap, void *d_proof_bad, fk_check_report *reports, double *check_ms);

#ifdef __cplusplus
}
#endif
#endif
