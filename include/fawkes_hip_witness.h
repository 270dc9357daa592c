/* Device witness generation of libfawkes_hip.so: the witness program of ONE instance of a batch circuit, run once per copy.
 *
 * The batch systems this library proves are `copies` instances of one gadget (fk_r1cs_load_tiled).  What the reference computes by
 * re-running the circuit closure on `WitnessCS` for every proof (prover.rs:69-76) is, for such a gadget, one straight-line program: every
 * auxiliary variable is a caller-supplied value or a fixed function of linear combinations of EARLIER variables.  The program is data
 * (this descriptor); csrc/witness.hip interprets it with one copy per lane and writes the witness in the tiled variable order, on the
 * library's stream, so fk_prove_r1cs_dev can be queued right behind it.
 *
 * These entry points are exported by the library and declared here, not in fawkes_hip.h: that header, its ctypes table and the Rust shim
 * describe one pinned ABI (tests/test_ffi_mirror.py); fawkes_hip_inspect.h is the precedent for a second header. */
#ifndef FAWKES_HIP_WITNESS_H
#define FAWKES_HIP_WITNESS_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* How auxiliary variable v gets its value (<l, z> = the linear combination l on this copy's ONE and aux variables): */
#define FK_WOP_GIVEN 0   /* row[arg0] of the copy's given row */
#define FK_WOP_MUL 1     /* <arg0, z> * <arg1, z>                          (CNum::mul, num.rs:247-262) */
#define FK_WOP_DIV0 2    /* <arg0, z> / <arg1, z>, 0 where the denominator is 0   (div_unchecked, num.rs:37-47) */
#define FK_WOP_INV0 3    /* 1 / <arg0, z>, 0 where it is 0                 (is_zero, num.rs:65-79) */
#define FK_WOP_BIT 4     /* bit arg1 (< 256) of the canonical value of <arg0, z>  (c_into_bits_le, bitify.rs:9-48) */

/* One instance.  Linear combinations live in one CSR table and are named by index, so an operation costs 9 bytes and a combination that
 * several operations share (the 254 bits of one signal) is stored once.  lc_col: 0 = ONE, 1 + j = Aux(j); no combination names a public
 * input other than ONE (the circuits define every input FROM an aux signal, `inputize`).  An operation on variable v may only name
 * combinations over Aux(j), j < v. */
typedef struct {
    uint32_t num_input, num_aux;      /* of one instance, num_input counts ONE */
    uint32_t n_given;                 /* elements of a copy's given row */
    uint32_t n_lc;
    const uint8_t *op;                /* [num_aux] FK_WOP_* */
    const uint32_t *arg0, *arg1;      /* [num_aux] */
    const uint32_t *input_lc;         /* [num_input - 1]: the combination that defines Input(1 + i) */
    const uint64_t *lc_ptr;           /* [n_lc + 1], lc_ptr[0] = 0, non-decreasing; an empty combination is 0 */
    const uint32_t *lc_col;           /* [nnz] */
    const uint64_t *lc_val;           /* [nnz * 4] Montgomery; NULL: every coefficient is ONE */
} fk_witness_desc;

typedef struct fk_witness_prog fk_witness_prog;

/* Host only, no GPU.  FK_ERR_BAD_ARG (the offending variable or combination named in fk_last_error(NULL)) for: an opcode outside the five,
 * a combination index >= n_lc, a column > num_aux, an operation on variable v whose combinations name Aux(j) with j >= v, a bit index
 * >= 256, a given index >= n_given, lc_ptr that does not start at 0 or decreases, num_input == 0, a missing array.  FK_ERR_FORMAT for a
 * coefficient image >= r.  This check is what lets the kernel index without bounds tests: a program that fails it never reaches the device. */
int fk_witness_program_check(const fk_witness_desc *desc);
/* checks, dictionary-codes the coefficients (8 bytes per term on the device, slot 0 = ONE) and uploads; the message of a refusal is in
 * fk_last_error(ctx) */
int fk_witness_program_load(fk_ctx *ctx, const fk_witness_desc *desc, fk_witness_prog **out);
/* out[8] = num_input, num_aux, n_given, combinations, terms, distinct coefficients (ONE included), combination evaluations per copy
 * (a run of consecutive BITs of one combination and a MUL of a combination by itself count once; the public inputs are included),
 * inversions per copy */
int fk_witness_program_info(const fk_witness_prog *prog, uint64_t out[8]);
void fk_witness_program_free(fk_ctx *ctx, fk_witness_prog *prog);
/* d_given: copies x n_given Montgomery elements, one row per copy (values below r: the caller's responsibility).  d_z receives
 * 1 + copies * (num_input - 1) + copies * num_aux elements in fk_r1cs_load_tiled's order: ONE, copy 0's inputs, copy 1's inputs, ...,
 * copy 0's aux, copy 1's aux, ...  Asynchronous on the library's stream.  copies == 0: nothing is written.  FK_ERR_BAD_ARG when the
 * batch does not fit 32-bit variable indices.  A witness that violates the circuit (a bad signature) is generated like any other. */
int fk_witness_generate_dev(fk_ctx *ctx, const fk_witness_prog *prog, const void *d_given, uint32_t copies, void *d_z);
/* the same with host buffers; blocks until z is written */
/* [staging] refused while a submitted proof's early front is outstanding (fk_prove_r1cs_submit) */
int fk_witness_generate(fk_ctx *ctx, const fk_witness_prog *prog, const uint64_t *given, uint32_t copies, uint64_t *z);

#ifdef __cplusplus
}
#endif
#endif
