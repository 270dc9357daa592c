// libfawkes_fieldtest.so: a TEST-ONLY device library (tests/test_gpu_field_ops.py, tests/test_gpu_point_ops.py; its second source,
// fieldtest_tower.hip, serves tests/test_tower_host.py and tests/test_gpu_tower_ops.py).  Not part of the product: it is not linked
// into libfawkes_hip.so and none of its symbols is part of the ABI (include/fawkes_hip.h).
//
// Every kernel is a thin wrapper: one thread loads the operands of one case, calls ONE method of field.hpp / curve.hpp exactly as
// the product spells it, and stores the result.  The methods under test are the device pass of the generated arithmetic
// (mont_mul_gfx950.inc, addsub_gfx950.inc), which no host code path executes.
//
// A case is `operands` elements in, `results` elements out, an element being one value of the type under test (8 x u32, or 16 for
// an Fq2 type: c0 || c1).  Point operations take their coordinates as consecutive elements (Xyzz: x y zz zzz; Affine: x y).
// Three kinds of operand are raw words in the first 8 words of an element, not field elements and not range-limited: the exponent of
// pow (8 words), the 64-bit argument of pow_u64 / from_u64 (words 0 and 1), and the scalar of a point multiplication (p_mul_scalar: 8
// words; p_mul_affine_bits: lo in words 0-1, hi in words 2-3, nbits in word 4, taken as at most 128).
//
// Modes -- the ways a wave-level carry chain can go wrong that operand values alone do not show:
//   straight : the operation, unconditionally (the caller picks n not a multiple of 64: a partial last wave)
//   divergent: lanes whose first operand is odd (bit 0 of its limb 0) run the operation, the others run ANOTHER operation
//              (alt_of) on the same operands: the SGPR-pair carries of both live under a partial EXEC mask
//   aliased  : the outputs overwrite the inputs in the same call, as curve.hpp does (F::mul2(zz, pp, zzz, ppp, zz, zzz))
#include "curve.hpp"
#include "fieldtest.hpp"
#include <stdio.h>
#include <type_traits>

using namespace fk;
using namespace ft;

namespace {

enum { T_FQ, T_FQL, T_FQC, T_FR, T_FRL, T_FQ2, T_FQ2L, T_FQ2C, T_COUNT };
enum {
    OP_ADD, OP_SUB, OP_DBL, OP_NEG, OP_ADD2, OP_SUB2, OP_ADDSUB2, OP_MUL, OP_SQR, OP_MUL2, OP_SQR2, OP_MULSUB, OP_DOT4,
    OP_IS_ZERO, OP_EQ, OP_CANON, OP_FROM_MONT, OP_TO_MONT,
    OP_P_ADD_MIXED, OP_P_ADD_MIXED_NZ, OP_P_ADD, OP_P_DBL, OP_P_DBL_AFFINE, OP_P_NEG_IF, OP_P_TO_AFFINE,
    // an id, once given, stays: new operations go to the end, so an older test file still names the kernels it means
    OP_INV, OP_POW, OP_POW_U64, OP_FROM_U64, OP_P_MUL_SCALAR, OP_P_MUL_AFFINE_BITS,
    OP_COUNT
};
enum { M_STRAIGHT, M_DIVERGENT, M_ALIASED, M_COUNT };

constexpr int nin_of(int op) {
    switch (op) {
    case OP_DBL: case OP_NEG: case OP_SQR: case OP_IS_ZERO: case OP_CANON: case OP_FROM_MONT: case OP_TO_MONT: case OP_INV: case OP_FROM_U64: return 1;
    case OP_ADD: case OP_SUB: case OP_MUL: case OP_SQR2: case OP_EQ: case OP_P_DBL_AFFINE: case OP_POW: case OP_POW_U64: return 2;
    case OP_P_NEG_IF: return 3;                                   // x, y, and an element whose limb 0 bit 0 is the flag
    case OP_P_MUL_AFFINE_BITS: return 3;                          // x, y, and an element holding lo, hi, nbits
    case OP_P_MUL_SCALAR: return 5;                               // Xyzz, and an element holding the scalar
    case OP_ADD2: case OP_SUB2: case OP_ADDSUB2: case OP_MUL2: case OP_MULSUB: case OP_P_DBL: case OP_P_TO_AFFINE: return 4;
    case OP_P_ADD_MIXED: case OP_P_ADD_MIXED_NZ: return 6;        // Xyzz accumulator, Affine addend
    case OP_DOT4: case OP_P_ADD: return 8;
    }
    return 0;
}
constexpr int nout_of(int op) {
    switch (op) {
    case OP_ADD2: case OP_SUB2: case OP_ADDSUB2: case OP_MUL2: case OP_SQR2: case OP_P_NEG_IF: case OP_P_TO_AFFINE: return 2;
    case OP_P_ADD_MIXED: case OP_P_ADD_MIXED_NZ: case OP_P_ADD: case OP_P_DBL: case OP_P_DBL_AFFINE:
    case OP_P_MUL_SCALAR: case OP_P_MUL_AFFINE_BITS: return 4;
    }
    return 1;
}
// the operation of the other arm in divergent mode (-1: the operation has no divergent form)
constexpr int alt_of(int op) {
    switch (op) {
    case OP_ADD: return OP_MUL;
    case OP_SUB: return OP_ADD;
    case OP_DBL: return OP_NEG;
    case OP_NEG: return OP_SQR;
    case OP_MUL: return OP_SUB;
    case OP_SQR: return OP_DBL;
    case OP_ADD2: return OP_SQR2;
    case OP_SUB2: return OP_ADD2;
    case OP_ADDSUB2: return OP_MUL2;
    case OP_MUL2: return OP_ADDSUB2;
    case OP_SQR2: return OP_SUB2;
    case OP_MULSUB: return OP_MUL2;
    case OP_DOT4: return OP_MULSUB;
    case OP_FROM_MONT: return OP_TO_MONT;
    case OP_TO_MONT: return OP_FROM_MONT;
    case OP_INV: return OP_POW;
    case OP_POW: return OP_INV;
    case OP_P_ADD_MIXED: case OP_P_ADD: return OP_P_DBL;
    }
    return -1;
}
constexpr bool aliasable(int op) {
    switch (op) {
    case OP_ADD: case OP_SUB: case OP_DBL: case OP_MUL: case OP_SQR: case OP_MULSUB:
    case OP_ADD2: case OP_SUB2: case OP_ADDSUB2: case OP_MUL2: case OP_SQR2: case OP_P_DBL: return true;
    }
    return false;
}

template <class F> struct Tr;
template <class P, bool INL> struct Tr<Fp<P, INL>> {
    static constexpr bool lazy = P::LAZY, fq2 = false, points = std::is_base_of<FqParams, P>::value;
    static constexpr int words = 8;
};
template <class B> struct Tr<Fq2T<B>> {
    static constexpr bool lazy = Tr<B>::lazy, fq2 = true, points = true;
    static constexpr int words = 16;
};
template <class F> constexpr bool supported(int op) {
    if (op < 0 || op >= OP_COUNT) return false;
    if (op == OP_DOT4) return !Tr<F>::lazy && !Tr<F>::fq2;
    if (op == OP_CANON) return Tr<F>::lazy;
    if (op == OP_FROM_MONT || op == OP_TO_MONT || op == OP_POW || op == OP_POW_U64 || op == OP_FROM_U64) return !Tr<F>::fq2;   // Fq2T has none of these
    if (op == OP_P_TO_AFFINE || op == OP_P_MUL_SCALAR || op == OP_P_MUL_AFFINE_BITS) return Tr<F>::points && !Tr<F>::lazy;
    if (op >= OP_P_ADD_MIXED && op <= OP_P_TO_AFFINE) return Tr<F>::points;
    return true;
}
template <class F> constexpr bool supported(int op, int mode) {
    if (!supported<F>(op)) return false;
    if (mode == M_STRAIGHT) return true;
    if (mode == M_DIVERGENT) return alt_of(op) >= 0 && supported<F>(alt_of(op));
    if (mode == M_ALIASED) return aliasable(op);
    return false;
}
constexpr int imax(int a, int b) { return a > b ? a : b; }

#if defined(__HIP_DEVICE_COMPILE__)
template <class P, bool INL> __device__ __forceinline__ void load(Fp<P, INL> &x, const uint32_t *p) {
#pragma unroll
    for (int i = 0; i < 8; i++) x.v[i] = p[i];
}
template <class B> __device__ __forceinline__ void load(Fq2T<B> &x, const uint32_t *p) { load(x.c0, p); load(x.c1, p + 8); }
template <class P, bool INL> __device__ __forceinline__ void store(uint32_t *p, const Fp<P, INL> &x) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = x.v[i];
}
template <class B> __device__ __forceinline__ void store(uint32_t *p, const Fq2T<B> &x) { store(p, x.c0); store(p + 8, x.c1); }
template <class P, bool INL> __device__ __forceinline__ uint32_t limb0(const Fp<P, INL> &x) { return x.v[0]; }
template <class B> __device__ __forceinline__ uint32_t limb0(const Fq2T<B> &x) { return x.c0.v[0]; }
// the first 8 words of an element, for the operands that are raw words
template <class P, bool INL> __device__ __forceinline__ const uint32_t *raw(const Fp<P, INL> &x) { return x.v; }
template <class B> __device__ __forceinline__ const uint32_t *raw(const Fq2T<B> &x) { return x.c0.v; }
__device__ __forceinline__ uint64_t raw64(const uint32_t *w) { return (uint64_t)w[1] << 32 | w[0]; }
template <class P, bool INL> __device__ __forceinline__ void set_flag(Fp<P, INL> &x, bool b) { x = Fp<P, INL>::zero(); x.v[0] = b ? 1u : 0u; }
template <class B> __device__ __forceinline__ void set_flag(Fq2T<B> &x, bool b) { x = Fq2T<B>::zero(); x.c0.v[0] = b ? 1u : 0u; }

template <class LP> __device__ __forceinline__ Fp<LP, true> canon_roundtrip(const Fp<LP, true> &a) { return lazy_of<LP>(canon(a)); }
__device__ __forceinline__ Fq2T<FqL> canon_roundtrip(const Fq2T<FqL> &a) {
    const Fq2T<Fq> c = canon(a);
    return Fq2T<FqL>{lazy_of<FqLazyParams>(c.c0), lazy_of<FqLazyParams>(c.c1)};
}

// one operation on the operands a[], results to r[].  AL: the outputs are written over the inputs by the call itself.
template <class F, int OP, bool AL>
__device__ __forceinline__ void apply(F *a, F *r) {
    if constexpr (OP == OP_ADD) { if constexpr (AL) { a[0] = F::add(a[0], a[1]); r[0] = a[0]; } else r[0] = F::add(a[0], a[1]); }
    else if constexpr (OP == OP_SUB) { if constexpr (AL) { a[1] = F::sub(a[0], a[1]); r[0] = a[1]; } else r[0] = F::sub(a[0], a[1]); }
    else if constexpr (OP == OP_DBL) { if constexpr (AL) { a[0] = F::dbl(a[0]); r[0] = a[0]; } else r[0] = F::dbl(a[0]); }
    else if constexpr (OP == OP_NEG) r[0] = F::neg(a[0]);
    else if constexpr (OP == OP_MUL) { if constexpr (AL) { a[1] = F::mul(a[0], a[1]); r[0] = a[1]; } else r[0] = F::mul(a[0], a[1]); }
    else if constexpr (OP == OP_SQR) { if constexpr (AL) { a[0] = F::sqr(a[0]); r[0] = a[0]; } else r[0] = F::sqr(a[0]); }
    else if constexpr (OP == OP_MULSUB) {      // curve.hpp: y = F::mulsub(r, F::sub(q_, x3), y, ppp)
        if constexpr (AL) { a[2] = F::mulsub(a[0], a[1], a[2], a[3]); r[0] = a[2]; } else r[0] = F::mulsub(a[0], a[1], a[2], a[3]);
    }
    else if constexpr (OP == OP_ADD2) { if constexpr (AL) { F::add2(a[0], a[1], a[2], a[3], a[0], a[2]); r[0] = a[0]; r[1] = a[2]; } else F::add2(a[0], a[1], a[2], a[3], r[0], r[1]); }
    else if constexpr (OP == OP_SUB2) { if constexpr (AL) { F::sub2(a[0], a[1], a[2], a[3], a[0], a[2]); r[0] = a[0]; r[1] = a[2]; } else F::sub2(a[0], a[1], a[2], a[3], r[0], r[1]); }
    else if constexpr (OP == OP_ADDSUB2) { if constexpr (AL) { F::addsub2(a[0], a[1], a[2], a[3], a[0], a[2]); r[0] = a[0]; r[1] = a[2]; } else F::addsub2(a[0], a[1], a[2], a[3], r[0], r[1]); }
    else if constexpr (OP == OP_MUL2) { if constexpr (AL) { F::mul2(a[0], a[1], a[2], a[3], a[0], a[2]); r[0] = a[0]; r[1] = a[2]; } else F::mul2(a[0], a[1], a[2], a[3], r[0], r[1]); }
    else if constexpr (OP == OP_SQR2) { if constexpr (AL) { F::sqr2(a[0], a[1], a[0], a[1]); r[0] = a[0]; r[1] = a[1]; } else F::sqr2(a[0], a[1], r[0], r[1]); }
    else if constexpr (OP == OP_DOT4) r[0] = F::dot4(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
    else if constexpr (OP == OP_IS_ZERO) set_flag(r[0], a[0].is_zero());
    else if constexpr (OP == OP_EQ) set_flag(r[0], a[0] == a[1]);
    else if constexpr (OP == OP_CANON) r[0] = canon_roundtrip(a[0]);
    else if constexpr (OP == OP_FROM_MONT) r[0] = F::from_mont(a[0]);
    else if constexpr (OP == OP_TO_MONT) r[0] = F::to_mont(a[0]);
    else if constexpr (OP == OP_INV) r[0] = F::inv(a[0]);
    else if constexpr (OP == OP_POW) r[0] = F::pow(a[0], raw(a[1]));
    else if constexpr (OP == OP_POW_U64) r[0] = F::pow_u64(a[0], raw64(raw(a[1])));
    else if constexpr (OP == OP_FROM_U64) r[0] = F::from_u64(raw64(raw(a[0])));
    else if constexpr (OP == OP_P_MUL_SCALAR) {
        const Xyzz<F> m = Xyzz<F>::mul_scalar(Xyzz<F>{a[0], a[1], a[2], a[3]}, raw(a[4]));
        r[0] = m.x; r[1] = m.y; r[2] = m.zz; r[3] = m.zzz;
    }
    else if constexpr (OP == OP_P_MUL_AFFINE_BITS) {
        const uint32_t *k = raw(a[2]);
        const Xyzz<F> m = Xyzz<F>::mul_affine_bits(Affine<F>{a[0], a[1]}, raw64(k), raw64(k + 2), k[4] < 128 ? (int)k[4] : 128);
        r[0] = m.x; r[1] = m.y; r[2] = m.zz; r[3] = m.zzz;
    }
    else if constexpr (OP == OP_P_ADD_MIXED || OP == OP_P_ADD_MIXED_NZ) {
        Xyzz<F> acc{a[0], a[1], a[2], a[3]};
        const Affine<F> q{a[4], a[5]};
        if constexpr (OP == OP_P_ADD_MIXED) acc.add_mixed(q); else acc.add_mixed_nz(q);
        r[0] = acc.x; r[1] = acc.y; r[2] = acc.zz; r[3] = acc.zzz;
    }
    else if constexpr (OP == OP_P_ADD) {
        Xyzz<F> acc{a[0], a[1], a[2], a[3]};
        acc.add(Xyzz<F>{a[4], a[5], a[6], a[7]});
        r[0] = acc.x; r[1] = acc.y; r[2] = acc.zz; r[3] = acc.zzz;
    }
    else if constexpr (OP == OP_P_DBL) {
        Xyzz<F> acc{a[0], a[1], a[2], a[3]};
        if constexpr (AL) { acc = Xyzz<F>::dbl(acc); r[0] = acc.x; r[1] = acc.y; r[2] = acc.zz; r[3] = acc.zzz; }
        else { const Xyzz<F> d = Xyzz<F>::dbl(acc); r[0] = d.x; r[1] = d.y; r[2] = d.zz; r[3] = d.zzz; }
    }
    else if constexpr (OP == OP_P_DBL_AFFINE) {
        const Xyzz<F> d = Xyzz<F>::dbl_affine(Affine<F>{a[0], a[1]});
        r[0] = d.x; r[1] = d.y; r[2] = d.zz; r[3] = d.zzz;
    }
    else if constexpr (OP == OP_P_NEG_IF) {
        const Affine<F> o = affine_neg_if(Affine<F>{a[0], a[1]}, (limb0(a[2]) & 1u) != 0);
        r[0] = o.x; r[1] = o.y;
    }
    else if constexpr (OP == OP_P_TO_AFFINE) {
        const Affine<F> o = Xyzz<F>{a[0], a[1], a[2], a[3]}.to_affine();
        r[0] = o.x; r[1] = o.y;
    }
}
#endif

// OPA: the operation; OPB: the other arm of divergent mode (== OPA in the other modes)
template <class F, int OPA, int OPB, int MODE>
__global__ void __launch_bounds__(256) ft_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int W = Tr<F>::words, NI = imax(nin_of(OPA), nin_of(OPB)), NO = imax(nout_of(OPA), nout_of(OPB));
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    F a[NI], r[NO];
#pragma unroll
    for (int j = 0; j < NI; j++) load(a[j], in + (i * NI + j) * W);
#pragma unroll
    for (int j = 0; j < NO; j++) r[j] = F::zero();
    if constexpr (MODE == M_DIVERGENT) {
        if (limb0(a[0]) & 1u) apply<F, OPA, false>(a, r);
        else apply<F, OPB, false>(a, r);
    } else {
        apply<F, OPA, MODE == M_ALIASED>(a, r);
    }
#pragma unroll
    for (int j = 0; j < NO; j++) store(out + (i * NO + j) * W, r[j]);
#endif
}

template <class F, int OPA, int OPB, int MODE>
int launch(const void *in, size_t operands, void *out, size_t results, size_t n) {
    constexpr int W = Tr<F>::words, NI = imax(nin_of(OPA), nin_of(OPB)), NO = imax(nout_of(OPA), nout_of(OPB));
    if (operands != (size_t)NI || results != (size_t)NO) {
        char d[128];
        snprintf(d, sizeof d, "a case has %d operands and %d results, got %zu and %zu", NI, NO, operands, results);
        return fail(FT_BAD_ARGUMENT, "ft_run", d);
    }
    if (n == 0 || n > (size_t)1 << 24) return fail(FT_BAD_ARGUMENT, "ft_run", "n out of range");
    return device_run(in, n * NI * W * 4, out, n * NO * W * 4, [n](uint32_t *din, uint32_t *dout) {
        ft_kernel<F, OPA, OPB, MODE><<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(din, dout, n);
    });
}

template <class F, int OP>
int run_op(int mode, const void *in, size_t operands, void *out, size_t results, size_t n) {
    if constexpr (supported<F>(OP, M_STRAIGHT)) if (mode == M_STRAIGHT) return launch<F, OP, OP, M_STRAIGHT>(in, operands, out, results, n);
    if constexpr (supported<F>(OP, M_DIVERGENT)) if (mode == M_DIVERGENT) return launch<F, OP, alt_of(OP), M_DIVERGENT>(in, operands, out, results, n);
    if constexpr (supported<F>(OP, M_ALIASED)) if (mode == M_ALIASED) return launch<F, OP, OP, M_ALIASED>(in, operands, out, results, n);
    return fail(FT_BAD_ARGUMENT, "ft_run", "the type has no such operation in this mode");
}

#define FT_OPS(X) \
    X(OP_ADD) X(OP_SUB) X(OP_DBL) X(OP_NEG) X(OP_ADD2) X(OP_SUB2) X(OP_ADDSUB2) X(OP_MUL) X(OP_SQR) X(OP_MUL2) X(OP_SQR2) X(OP_MULSUB) X(OP_DOT4) \
    X(OP_IS_ZERO) X(OP_EQ) X(OP_CANON) X(OP_FROM_MONT) X(OP_TO_MONT) X(OP_INV) X(OP_POW) X(OP_POW_U64) X(OP_FROM_U64) \
    X(OP_P_ADD_MIXED) X(OP_P_ADD_MIXED_NZ) X(OP_P_ADD) X(OP_P_DBL) X(OP_P_DBL_AFFINE) X(OP_P_NEG_IF) X(OP_P_TO_AFFINE) \
    X(OP_P_MUL_SCALAR) X(OP_P_MUL_AFFINE_BITS)

template <class F>
int run_type(int op, int mode, const void *in, size_t operands, void *out, size_t results, size_t n) {
    switch (op) {
#define X(o) case o: return run_op<F, o>(mode, in, operands, out, results, n);
        FT_OPS(X)
#undef X
    }
    return fail(FT_BAD_ARGUMENT, "ft_run", "unknown operation");
}

#define FT_TYPES(X) X(T_FQ, Fq) X(T_FQL, FqL) X(T_FQC, FqC) X(T_FR, Fr) X(T_FRL, FrL) X(T_FQ2, Fq2) X(T_FQ2L, Fq2T<FqL>) X(T_FQ2C, Fq2C)

}  // namespace

namespace ft {
char g_err[512] = "";
bool g_failed = false;
int fail(int code, const char *what, const char *detail) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, detail);
    if (code == FT_HIP_ERROR) g_failed = true;
    return code;
}
}  // namespace ft

extern "C" {

const char *ft_last_error(void) { return g_err; }

// 32-bit words of one element of the type (8, or 16 for an Fq2 type); 0 for an unknown type
int ft_elem_words(int type) {
    switch (type) {
#define X(t, F) case t: return Tr<F>::words;
        FT_TYPES(X)
#undef X
    }
    return 0;
}

// 1 if ft_run accepts (type, op, mode), and then the elements per case it expects
int ft_supported(int type, int op, int mode, int *operands, int *results) {
    bool ok = false;
    switch (type) {
#define X(t, F) case t: ok = supported<F>(op, mode); break;
        FT_TYPES(X)
#undef X
    }
    if (!ok) return 0;
    const int alt = mode == M_DIVERGENT ? alt_of(op) : op;
    if (operands) *operands = imax(nin_of(op), nin_of(alt));
    if (results) *results = imax(nout_of(op), nout_of(alt));
    return 1;
}

// the other arm of divergent mode, -1 if none
int ft_alt_op(int op) { return alt_of(op); }

// n cases of (type, op) in `mode` on device 0: 256-thread blocks, synchronous.  Returns 0, or a code with ft_last_error() set;
// never aborts.  After a HIP error every further call returns FT_AFTER_ERROR without touching the device.
int ft_run(int type, int op, int mode, const void *in, size_t operands, void *out, size_t results, size_t n) {
    if (g_failed) return FT_AFTER_ERROR;
    if (!in || !out) return fail(FT_BAD_ARGUMENT, "ft_run", "null buffer");
    switch (type) {
#define X(t, F) case t: return run_type<F>(op, mode, in, operands, out, results, n);
        FT_TYPES(X)
#undef X
    }
    return fail(FT_BAD_ARGUMENT, "ft_run", "unknown type");
}

}  // extern "C"
