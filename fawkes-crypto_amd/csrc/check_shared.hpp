// What the two R1CS checks share (check.hip: one large system; batch_check.hip: many proofs of one small one): the sentinel, the two
// predicates a verdict is made of, and the host references' walk over one row of the CSR.  One definition each, so that the device
// kernels and the host references of both paths cannot drift apart.
#pragma once
#include <string.h>
#include "common.hpp"

namespace fk {

static constexpr unsigned long long CHECK_NONE = ~0ull;

// the 256-bit image is below r (the borrow of x - r)
static FK_HD bool image_below_r(const Fr &x) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)x.v[i] - FrParams::p(i) - br;
        br = (uint32_t)(t >> 63);
    }
    return br != 0;
}

// The gate a * b = c is violated: one Montgomery product, then a limb compare with c.  field.hpp keeps every value canonical (Fr::mul
// ends with the conditional subtraction, the evaluation's sums reduce below r), so equality in the field IS equality of the eight
// limbs -- no subtraction, no second representative to try.
static FK_HD bool product_differs(const Fr &a, const Fr &b, const Fr &c) { return Fr::mul(a, b) != c; }

// ---- host references: one matrix of a fk_r1cs and <row, z> with the arithmetic of fk_synthesize
struct CsrView { const uint64_t *ptr; const uint32_t *col; const uint64_t *val; };

// the three matrices of a system whose pointers are present and whose variable indices are below num_input + num_aux
static inline int check_host_system(fk_ctx *ctx, const fk_r1cs *cs, CsrView mats[3]) {
    if (!cs->num_input) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: a system has the input ONE");
    mats[0] = {cs->a_ptr, cs->a_col, cs->a_val}; mats[1] = {cs->b_ptr, cs->b_col, cs->b_val}; mats[2] = {cs->c_ptr, cs->c_col, cs->c_val};
    const uint64_t nv = (uint64_t)cs->num_input + cs->num_aux;
    for (int m = 0; m < 3; m++) {
        if (!mats[m].ptr) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "check: null row pointer");
        for (uint64_t k = mats[m].ptr[0]; k < mats[m].ptr[cs->num_gates]; k++)
            if (mats[m].col[k] >= nv) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs: variable index %u out of range", mats[m].col[k]);
    }
    return FK_OK;
}

// <row, z>: a unit coefficient is not multiplied, the terms are added in row order.  where(v): the place of instance variable v in z.
template <class Where>
static inline Fr csr_row_dot(const CsrView &mt, uint64_t row, const Fr *z, Where where) {
    const Fr one = Fr::one();
    Fr acc = Fr::zero();
    for (uint64_t k = mt.ptr[row]; k < mt.ptr[row + 1]; k++) {
        Fr t = z[where(mt.col[k])];
        if (mt.val) {                  // NULL: every coefficient of this matrix is ONE
            Fr cf; memcpy(&cf, mt.val + 4 * k, 32);
            if (cf != one) t = Fr::mul(t, cf);
        }
        acc = Fr::add(acc, t);
    }
    return acc;
}

}  // namespace fk
