/* The R1CS check of libfawkes_hip.so: which gates, and which copies of a batch circuit, a witness violates.
 *
 * The prover's bytes are defined for any witness (a bad signature is proved like any other, and the proof then fails to verify); the
 * reference finds the offending gate with its debugging constraint system, which asserts a * b == c per gate (circuit/r1cs/cs.rs:157,
 * "Not satisfied constraint").  Here the same test runs on the device over the a = A z, b = B z, c = C z the prover evaluates anyway
 * (csrc/check.hip): one gate per lane, a bitmap of the bad gates, one flag per group of consecutive gates (per copy of a tiled system),
 * and the witness's own sanity -- every element below r, z[0] = ONE.
 *
 * These entry points are exported by the library and declared here, not in fawkes_hip.h: that header, its ctypes table and the Rust shim
 * describe one pinned ABI (tests/test_ffi_mirror.py); fawkes_hip_witness.h and fawkes_hip_verify.h are the precedent. */
#ifndef FAWKES_HIP_CHECK_H
#define FAWKES_HIP_CHECK_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FK_CHECK_NONE UINT64_MAX
typedef struct {
    uint64_t gates;           /* gate rows examined: num_gates of the system, all copies (the per-input rows "input_i * 0 = 0" hold by construction and are not counted) */
    uint64_t n_bad;           /* gates with <A_i,z> * <B_i,z> != <C_i,z> in Fr */
    uint64_t first_bad;       /* the lowest such gate, FK_CHECK_NONE if none */
    uint64_t first_abc[3][4]; /* <A,z>, <B,z>, <C,z> of that gate, Montgomery; zeros if none */
    uint64_t n_groups, n_bad_groups;   /* group_rows > 0: ceil(gates / group_rows) and how many hold a bad gate; else 0, 0 */
    uint64_t n_range;         /* witness elements whose 256-bit image is >= r */
    uint64_t first_range;     /* the lowest such variable index, FK_CHECK_NONE if none */
    int32_t  one_ok;          /* z[0] is the Montgomery image of ONE */
    int32_t  gates_valid;     /* 0 when n_range > 0: field arithmetic is defined for images below r only, so the gate fields,
                                 the bitmap and the group flags are then unspecified (but written within their bounds) */
} fk_check_report;            /* padding bytes zero */

/* Outputs of all three calls: bad_bitmap holds ceil(gates / 64) words, bit g % 64 of word g / 64 set iff gate g is bad, the bits at and
 * beyond `gates` zero; group_bad holds n_groups bytes, 0 or 1, group k = the gates [k * group_rows, (k + 1) * group_rows) -- for a tiled
 * system group_rows = the gates of one instance gives one flag per copy.  Either may be NULL.  Nothing outside these extents is written;
 * every output is deterministic.  FK_ERR_BAD_ARG for a null report, system or witness and for group_bad without group_rows.  A violated
 * system is NOT an error: the call returns FK_OK and the report speaks. */

/* host, ctx may be NULL, no GPU: the reference the device entry is compared with.  cs = one instance, copies >= 1 in
 * fk_r1cs_load_tiled's variable and row order (1 = the system itself); copies == 0 is FK_ERR_BAD_ARG. */
int fk_r1cs_check(fk_ctx *ctx, const fk_r1cs *cs, uint32_t copies, const uint64_t *z, uint64_t group_rows,
                  uint64_t *bad_bitmap, uint8_t *group_bad, fk_check_report *report);
/* device: d_z as for fk_prove_r1cs_dev; d_bad_bitmap / d_group_bad are device pointers, either may be NULL; report is a host
 * pointer; blocks until it is filled. */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_r1cs_check_dev(fk_ctx *ctx, const fk_r1cs_dev *r1cs, const void *d_z, uint64_t group_rows,
                      void *d_bad_bitmap, void *d_group_bad, fk_check_report *report);
/* fk_prove_r1cs_dev plus the check of the SAME evaluation: the check kernels run on the evaluated a, b, c between the
 * evaluation and the quotient; the proof bytes are those of fk_prove_r1cs_dev whether or not the witness satisfies the
 * system (the prover's bytes are defined for any witness); the report is read when the proof is.  Key and system mismatches are
 * reported as fk_prove_r1cs_dev reports them.  The call does not join the fk_prove_r1cs_submit / _wait pipeline: an outstanding
 * early front of that pipeline is refused (FK_ERR_BAD_ARG) the way fk_prove_r1cs_dev refuses a foreign one. */
int fk_prove_r1cs_checked_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r1cs, const void *d_z, const uint64_t r[4],
                              const uint64_t s[4], uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm, uint64_t group_rows,
                              void *d_bad_bitmap, void *d_group_bad, fk_check_report *report);

#ifdef __cplusplus
}
#endif
#endif
