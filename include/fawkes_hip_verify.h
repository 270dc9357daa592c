/* Aggregated Groth16 batch verification of libfawkes_hip.so: `count` proofs of one key checked by ONE pairing equation.
 *
 * fk_verify_batch_dev (fawkes_hip.h) checks e(A_i, B_i) = e(alpha, beta) e(acc_i, gamma) e(C_i, delta) proof by proof: four Miller loops
 * and a final exponentiation each.  With secret nonzero 128-bit weights w_i all `count` equations hold iff
 *
 *     prod_i e(w_i A_i, B_i) * e(-(sum_i w_i) alpha, beta) * e(-S_acc, gamma) * e(-S_C, delta) = 1
 *     S_C = sum_i w_i C_i,    S_acc = (sum_i w_i) ic_0 + sum_j (sum_i w_i x_ij) ic_j
 *
 * except with probability about 2^-128 over the weights: one Miller loop and two 128-bit G1 multiplications per proof, three Miller
 * loops and one final exponentiation per batch (csrc/verify_agg.hip, csrc/pairing.hpp: miller_loop_proj).
 *
 * SOUNDNESS RESTS ON THE WEIGHTS: they must not be known to -- or predictable by -- whoever made the proofs.  A party that knows them
 * can submit proofs that are each invalid and whose errors cancel in the sum.  Pass weights = NULL (the library draws them from
 * getrandom(2) for every call) unless you are testing; never reuse or publish explicit weights.
 *
 * These entry points are exported by the library and declared here, not in fawkes_hip.h: that header, its ctypes table and the Rust shim
 * describe one pinned ABI (tests/test_ffi_mirror.py); fawkes_hip_witness.h is the precedent for a further header. */
#ifndef FAWKES_HIP_VERIFY_H
#define FAWKES_HIP_VERIFY_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t count, n_wellformed;
    int32_t  equation_ok;     /* the aggregated equation over the well-formed proofs (1 when there are none) */
    uint64_t sum_w[4];        /* sum of w_i mod r over the well-formed proofs, Montgomery */
    uint8_t  s_acc[64], s_c[64];   /* raw affine Montgomery LE, zeros = identity, as FK_G1_BYTES everywhere */
} fk_verify_agg_report;

/* vk, inputs (count x n_inputs Montgomery Fr, without the leading ONE) and proofs (count x FK_PROOF_BYTES) as for fk_verify_batch_dev.
 * weights: count x 2 u64, little-endian 128-bit, each nonzero (a zero weight would silently drop a proof: FK_ERR_BAD_ARG); NULL: the
 *     library draws them -- 32 bytes of getrandom(2) (FK_ERR_UNSUPPORTED if that fails) key a ChaCha20 stream, zero draws are redrawn.
 * wellformed (count bytes, may be NULL): 0 for a proof with a coordinate >= q, A or C off the curve, or B off the twist or outside the
 *     order-r subgroup -- the checks of fk_verify.  Such a proof contributes nothing: its weight is left out of all three sums and its
 *     Miller value is one.  It never makes the call fail; fk_last_error names the first one.
 * *accept = equation_ok && n_wellformed == count.  count == 0: accept = 1.  A verifying key with a coordinate >= q leaves no proof
 *     well-formed (fk_verify_batch_dev rejects every proof under such a key).  FK_ERR_FORMAT / FK_ERR_KEY_MISMATCH for the key's framing
 *     and the input count as in fk_verify_batch_dev.
 * report (may be NULL): see above; padding bytes are zero.
 * An accepted batch means every proof verifies.  A rejected one says nothing about WHICH proof is bad: run fk_verify_batch_dev on the
 * well-formed ones (fawkes_crypto_amd.verify_agg.verify_batch_aggregated does).
 *
 * fk_verify_aggregate runs on the host (ctx may be NULL, no GPU needed): the reference the device entry is compared with, some
 * milliseconds per proof on one core.  fk_verify_aggregate_dev runs the per-proof part on the GPU, one proof per lane, and the
 * per-batch tail (the sums in Fr, n_ic scalar multiplications, three Miller loops, the final exponentiation: a fixed cost of some
 * milliseconds) on the host; all pointers are host pointers; it blocks until the verdict is known. */
int fk_verify_aggregate(fk_ctx *ctx, const uint8_t *vk, size_t vk_len, const uint64_t *inputs, uint32_t n_inputs, const uint8_t *proofs,
                        uint32_t count, const uint64_t *weights, uint8_t *wellformed, int *accept, fk_verify_agg_report *report);
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_verify_aggregate_dev(fk_ctx *ctx, const uint8_t *vk, size_t vk_len, const uint64_t *inputs, uint32_t n_inputs, const uint8_t *proofs,
                            uint32_t count, const uint64_t *weights, uint8_t *wellformed, int *accept, fk_verify_agg_report *report);

#ifdef __cplusplus
}
#endif
#endif
