// What powers.hip's kernels and its host references share, and all that the references are made of: the generators and curve constants
// per coordinate field, the classes of a point, the scale loop.  A header of its own so that the references can be compiled into a
// stand-alone host program (tools/powers_host_check.hip) without the library.
#pragma once
#include "ceremony_shared.hpp"

namespace fk {

// the group's generator and the curve's b per coordinate field, usable in a kernel
template <class F> struct CurveOf;
template <> struct CurveOf<Fq> {
    static constexpr bool HAS_COFACTOR = false;
    static FK_HD G1Affine gen() { return G1Affine{Fq::one(), Fq::dbl(Fq::one())}; }
    static FK_HD Fq b() { const uint32_t w[8] = FK_G1_B; Fq t; for (int i = 0; i < 8; i++) t.v[i] = w[i]; return t; }
};
template <> struct CurveOf<Fq2> {
    static constexpr bool HAS_COFACTOR = true;
    static FK_HD G2Affine gen() {
        const uint32_t x0[8] = FK_G2_GEN_X0, x1[8] = FK_G2_GEN_X1, y0[8] = FK_G2_GEN_Y0, y1[8] = FK_G2_GEN_Y1;
        G2Affine g;
        for (int i = 0; i < 8; i++) { g.x.c0.v[i] = x0[i]; g.x.c1.v[i] = x1[i]; g.y.c0.v[i] = y0[i]; g.y.c1.v[i] = y1[i]; }
        return g;
    }
    static FK_HD Fq2 b() {
        const uint32_t b0[8] = FK_G2_B0, b1[8] = FK_G2_B1;
        Fq2 t;
        for (int i = 0; i < 8; i++) { t.c0.v[i] = b0[i]; t.c1.v[i] = b1[i]; }
        return t;
    }
};

// ---- the classes of a point, in the order they are tested
enum PointClass : int { PT_GOOD = 0, PT_INFINITY = 1, PT_RANGE = 2, PT_CURVE = 3, PT_SUBGROUP = 4 };

static FK_HD bool limbs_below_q(const Fq &a) {
    bool below = false, decided = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const uint32_t q = FqParams::p(i);
        if (!decided && a.v[i] != q) { below = a.v[i] < q; decided = true; }
    }
    return below;
}
static FK_HD bool limbs_below_q(const Fq2 &a) { return limbs_below_q(a.c0) && limbs_below_q(a.c1); }

// infinity, range or curve; PT_GOOD says "on the curve": the subgroup is the caller's (it costs a multiplication by r)
template <class F>
static FK_HD PointClass point_class_on_curve(const Affine<F> &p) {
    if (p.is_inf()) return PT_INFINITY;
    if (!(limbs_below_q(p.x) && limbs_below_q(p.y))) return PT_RANGE;
    const F rhs = F::add(F::mul(F::sqr(p.x), p.x), CurveOf<F>::b());
    if (F::sqr(p.y) != rhs) return PT_CURVE;
    return PT_GOOD;
}

static inline Fr r_as_limbs() {
    const uint32_t w[8] = FK_R_CANON;
    Fr r;
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}

// ---- the host references: plain loops over the generic double-and-add
template <class F>
static PointClass host_point_class(const Affine<F> &p) {
    const PointClass c = point_class_on_curve<F>(p);
    if (c != PT_GOOD || !CurveOf<F>::HAS_COFACTOR) return c;
    return Xyzz<F>::mul_scalar(Xyzz<F>::from_affine(p), r_as_limbs().v).is_inf() ? PT_GOOD : PT_SUBGROUP;
}

struct PointsCount { unsigned long long infinity, range, curve, subgroup, first_bad; };      // fk_points_report, as the atomics want it

template <class F>
static void host_points_validate(const uint8_t *pts, uint64_t n, PointsCount *rep) {
    *rep = PointsCount{0, 0, 0, 0, ~0ull};
    for (uint64_t i = 0; i < n; i++) {
        Affine<F> p;
        memcpy(&p, pts + sizeof(Affine<F>) * i, sizeof p);
        const PointClass c = host_point_class<F>(p);
        if (c == PT_GOOD) continue;
        (c == PT_INFINITY ? rep->infinity : c == PT_RANGE ? rep->range : c == PT_CURVE ? rep->curve : rep->subgroup)++;
        if (rep->first_bad == ~0ull) rep->first_bad = i;
    }
}

// out[i] = [c x^(first + i)] in[i]; out may be in
template <class F>
static void host_scale_powers(const uint8_t *in, uint64_t n, uint64_t first, const Fr &x, const Fr &c, uint8_t *out) {
    Fr k = Fr::mul(Fr::pow_u64(x, first), c);
    for (uint64_t i = 0; i < n; i++) {
        Affine<F> p;
        memcpy(&p, in + sizeof(Affine<F>) * i, sizeof p);
        p = host_mul<F>(p, k);
        memcpy(out + sizeof(Affine<F>) * i, &p, sizeof p);
        k = Fr::mul(k, x);
    }
}

}  // namespace fk
