// The second source of the TEST-ONLY library libfawkes_fieldtest.so (fieldtest.hip): the pairing tower of pairing.hpp by value, for
// tests/test_tower_host.py and tests/test_gpu_tower_ops.py.  Not part of the product.
//
// The rules of fieldtest.hip hold: a wrapper loads the operands of one case, calls ONE function of pairing.hpp exactly as the product
// spells it, and stores the result.  The wrapper body is one FK_HD template, tower_case<F, OP>:
//   device: one thread per case in 64-thread blocks (__launch_bounds__(64), as verify_batch_kernel and agg_miller_kernel), F = FqC, the
//           only type the device pairing code uses;
//   host  : a plain loop with F = Fq, the type fk_verify uses.  The host arm makes no HIP call: it runs on a machine without a GPU.
//
// A case is words_in 32-bit words in and words_out out (ft_tower_shape).  Elements are Montgomery limb images: Fq2 = c0 || c1 (16
// words), Fq6 = c0 c1 c2 (48), Fq12 = c0 || c1 (96), an affine G1 point x y (16), an affine G2 point x y (32).  f12_pow takes its
// exponent as 24 raw words and the `nwords` argument from a 25th (taken as at most 24); f12_is_one returns one word, 0 or 1.
#include "pairing.hpp"
#include "fieldtest.hpp"
#include <stdio.h>
#include <string.h>

using namespace fk;
using namespace ft;

namespace {

enum {
    TW_F6_MUL, TW_F6_MUL_BY_01, TW_F6_MUL_BY_FQ2, TW_F6_MUL_V, TW_F6_MUL_XI, TW_F6_INV, TW_F6_ADD, TW_F6_SUB, TW_F6_NEG,
    TW_F12_MUL, TW_F12_SQR_COMPLEX, TW_F12_MUL_BY_LINE, TW_F12_CONJ, TW_F12_INV, TW_F12_IS_ONE, TW_F12_POW,
    TW_MILLER_LOOP, TW_MILLER_LOOP_PROJ, TW_FINAL_EXP, TW_COUNT
};
enum { WHERE_DEVICE, WHERE_HOST };
constexpr int W2 = 16, W6 = 48, W12 = 96, POW_WORDS = 24;

constexpr int words_in_of(int op) {
    switch (op) {
    case TW_F6_MUL: case TW_F6_ADD: case TW_F6_SUB: return 2 * W6;
    case TW_F6_MUL_BY_01: return W6 + 2 * W2;
    case TW_F6_MUL_BY_FQ2: return W6 + W2;
    case TW_F6_MUL_V: case TW_F6_INV: case TW_F6_NEG: return W6;
    case TW_F6_MUL_XI: return W2;
    case TW_F12_MUL: return 2 * W12;
    case TW_F12_MUL_BY_LINE: return W12 + 3 * W2;
    case TW_F12_SQR_COMPLEX: case TW_F12_CONJ: case TW_F12_INV: case TW_F12_IS_ONE: case TW_FINAL_EXP: return W12;
    case TW_F12_POW: return W12 + POW_WORDS + 1;
    case TW_MILLER_LOOP: case TW_MILLER_LOOP_PROJ: return 16 + 32;
    }
    return 0;
}
constexpr int words_out_of(int op) {
    if (op < 0 || op >= TW_COUNT) return 0;
    if (op <= TW_F6_NEG) return op == TW_F6_MUL_XI ? W2 : W6;
    return op == TW_F12_IS_ONE ? 1 : W12;
}

template <class F> FK_HD F ld(const uint32_t *p) { F x; for (int i = 0; i < 8; i++) x.v[i] = p[i]; return x; }
template <class F> FK_HD Fq2T<F> ld2(const uint32_t *p) { return Fq2T<F>{ld<F>(p), ld<F>(p + 8)}; }
template <class F> FK_HD Fq6T<F> ld6(const uint32_t *p) { return Fq6T<F>{ld2<F>(p), ld2<F>(p + W2), ld2<F>(p + 2 * W2)}; }
template <class F> FK_HD Fq12T<F> ld12(const uint32_t *p) { return Fq12T<F>{ld6<F>(p), ld6<F>(p + W6)}; }
template <class F> FK_HD void st(uint32_t *p, const F &x) { for (int i = 0; i < 8; i++) p[i] = x.v[i]; }
template <class F> FK_HD void st(uint32_t *p, const Fq2T<F> &x) { st(p, x.c0); st(p + 8, x.c1); }
template <class F> FK_HD void st(uint32_t *p, const Fq6T<F> &x) { st(p, x.c0); st(p + W2, x.c1); st(p + 2 * W2, x.c2); }
template <class F> FK_HD void st(uint32_t *p, const Fq12T<F> &x) { st(p, x.c0); st(p + W6, x.c1); }

// one case of one operation: `in` and `out` are the case's own words
template <class F, int OP>
FK_HD void tower_case(const uint32_t *in, uint32_t *out) {
    using F6 = Fq6T<F>; using F12 = Fq12T<F>;
    if constexpr (OP == TW_F6_MUL) st(out, F6::mul(ld6<F>(in), ld6<F>(in + W6)));
    else if constexpr (OP == TW_F6_MUL_BY_01) st(out, F6::mul_by_01(ld6<F>(in), ld2<F>(in + W6), ld2<F>(in + W6 + W2)));
    else if constexpr (OP == TW_F6_MUL_BY_FQ2) st(out, F6::mul_by_fq2(ld6<F>(in), ld2<F>(in + W6)));
    else if constexpr (OP == TW_F6_MUL_V) st(out, F6::mul_v(ld6<F>(in)));
    else if constexpr (OP == TW_F6_MUL_XI) st(out, F6::mul_xi(ld2<F>(in)));
    else if constexpr (OP == TW_F6_INV) st(out, F6::inv(ld6<F>(in)));
    else if constexpr (OP == TW_F6_ADD) st(out, F6::add(ld6<F>(in), ld6<F>(in + W6)));
    else if constexpr (OP == TW_F6_SUB) st(out, F6::sub(ld6<F>(in), ld6<F>(in + W6)));
    else if constexpr (OP == TW_F6_NEG) st(out, F6::neg(ld6<F>(in)));
    else if constexpr (OP == TW_F12_MUL) st(out, F12::mul(ld12<F>(in), ld12<F>(in + W12)));
    else if constexpr (OP == TW_F12_SQR_COMPLEX) st(out, F12::sqr_complex(ld12<F>(in)));
    else if constexpr (OP == TW_F12_MUL_BY_LINE) st(out, F12::mul_by_line(ld12<F>(in), ld2<F>(in + W12), ld2<F>(in + W12 + W2), ld2<F>(in + W12 + 2 * W2)));
    else if constexpr (OP == TW_F12_CONJ) st(out, F12::conj(ld12<F>(in)));
    else if constexpr (OP == TW_F12_INV) st(out, F12::inv(ld12<F>(in)));
    else if constexpr (OP == TW_F12_IS_ONE) out[0] = ld12<F>(in).is_one() ? 1u : 0u;
    else if constexpr (OP == TW_F12_POW) {
        const uint32_t nwords = in[W12 + POW_WORDS];
        st(out, F12::pow(ld12<F>(in), in + W12, nwords < POW_WORDS ? (int)nwords : POW_WORDS));    // the exponent is read where it lies
    }
    else if constexpr (OP == TW_MILLER_LOOP) st(out, miller_loop<F>(Affine<F>{ld<F>(in), ld<F>(in + 8)}, Affine<Fq2T<F>>{ld2<F>(in + 16), ld2<F>(in + 32)}));
    else if constexpr (OP == TW_MILLER_LOOP_PROJ) st(out, miller_loop_proj<F>(Affine<F>{ld<F>(in), ld<F>(in + 8)}, Affine<Fq2T<F>>{ld2<F>(in + 16), ld2<F>(in + 32)}));
    else if constexpr (OP == TW_FINAL_EXP) st(out, final_exponentiation<F>(ld12<F>(in)));
}

template <int OP>
__global__ void __launch_bounds__(64) tw_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    tower_case<FqC, OP>(in + i * words_in_of(OP), out + i * words_out_of(OP));
#endif
}

template <int OP>
int run_tower(int where, const uint32_t *in, uint32_t *out, size_t n) {
    constexpr size_t WI = words_in_of(OP), WO = words_out_of(OP);
    if (where == WHERE_HOST) {
        memset(out, 0xee, n * WO * 4);
        for (size_t i = 0; i < n; i++) tower_case<Fq, OP>(in + i * WI, out + i * WO);
        return FT_OK;
    }
    return device_run(in, n * WI * 4, out, n * WO * 4, [n](uint32_t *din, uint32_t *dout) {
        tw_kernel<OP><<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(din, dout, n);
    });
}

#define TW_OPS(X) \
    X(TW_F6_MUL) X(TW_F6_MUL_BY_01) X(TW_F6_MUL_BY_FQ2) X(TW_F6_MUL_V) X(TW_F6_MUL_XI) X(TW_F6_INV) X(TW_F6_ADD) X(TW_F6_SUB) X(TW_F6_NEG) \
    X(TW_F12_MUL) X(TW_F12_SQR_COMPLEX) X(TW_F12_MUL_BY_LINE) X(TW_F12_CONJ) X(TW_F12_INV) X(TW_F12_IS_ONE) X(TW_F12_POW) \
    X(TW_MILLER_LOOP) X(TW_MILLER_LOOP_PROJ) X(TW_FINAL_EXP)

}  // namespace

extern "C" {

// 1 if `op` is a tower operation, and then the 32-bit words of one case in and out
int ft_tower_shape(int op, int *words_in, int *words_out) {
    if (op < 0 || op >= TW_COUNT) return 0;
    if (words_in) *words_in = words_in_of(op);
    if (words_out) *words_out = words_out_of(op);
    return 1;
}

// n cases of `op`: where = 0 on device 0 (one thread per case, 64-thread blocks, synchronous), where = 1 on the host (no HIP call).
// The error contract of ft_run: returns 0, or a code with ft_last_error() set; never aborts; the output is 0xee-filled before the
// run; after a HIP error every further device call returns FT_AFTER_ERROR without touching the device.
int ft_tower_run(int op, int where, const void *in, size_t words_in, void *out, size_t words_out, size_t n) {
    if (where != WHERE_DEVICE && where != WHERE_HOST) return fail(FT_BAD_ARGUMENT, "ft_tower_run", "where is 0 (device) or 1 (host)");
    if (where == WHERE_DEVICE && g_failed) return FT_AFTER_ERROR;
    if (!in || !out) return fail(FT_BAD_ARGUMENT, "ft_tower_run", "null buffer");
    if (op < 0 || op >= TW_COUNT) return fail(FT_BAD_ARGUMENT, "ft_tower_run", "unknown operation");
    if (words_in != (size_t)words_in_of(op) || words_out != (size_t)words_out_of(op)) {
        char d[128];
        snprintf(d, sizeof d, "a case has %d words in and %d out, got %zu and %zu", words_in_of(op), words_out_of(op), words_in, words_out);
        return fail(FT_BAD_ARGUMENT, "ft_tower_run", d);
    }
    if (n == 0 || n > (size_t)1 << 16) return fail(FT_BAD_ARGUMENT, "ft_tower_run", "n out of range");
    switch (op) {
#define X(o) case o: return run_tower<o>(where, (const uint32_t *)in, (uint32_t *)out, n);
        TW_OPS(X)
#undef X
    }
    return fail(FT_BAD_ARGUMENT, "ft_tower_run", "unknown operation");
}

}  // extern "C"
