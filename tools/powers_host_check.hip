// Stand-alone host check of the references in csrc/powers_host.hpp, for a sanitizer build (no library, no GPU, no Python):
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I fawkes-crypto_amd/csrc tools/powers_host_check.hip -o powers_host_check
// Compares, on a few hundred scalar / point pairs per group: the scale loop with Xyzz::mul_scalar of c x^(first + i) computed
// independently; mul_naf of naf_recode(k) and mul_affine_k256 with mul_scalar; naf_recode(r) feeding mul_naf<Fq2> on points inside and
// outside the subgroup; the validate predicates on points of every class.  Exit status 0 and "ok" when everything agrees.
#include "powers_host.hpp"
#include <stdio.h>

using namespace fk;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static Fr rand_fr() {      // a Montgomery image below r: the top two bits shaved, retried
    for (;;) {
        Fr k;
        for (int i = 0; i < 8; i++) k.v[i] = (uint32_t)rng();
        k.v[7] &= 0x3fffffffu;
        bool below = false;
        for (int i = 7; i >= 0; i--) { if (k.v[i] != FrParams::p(i)) { below = k.v[i] < FrParams::p(i); break; } }
        if (below && !k.is_zero()) return k;
    }
}

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED: %s (line %d)\n", what, __LINE__); } } while (0)

template <class F>
static bool same(const Affine<F> &a, const Affine<F> &b) { return !memcmp(&a, &b, sizeof a); }

template <class F>
static void check_group(const char *name, int n) {
    const Affine<F> gen = CurveOf<F>::gen();
    std::vector<Affine<F>> pts(n);
    for (int i = 0; i < n; i++) pts[i] = host_mul<F>(gen, rand_fr());
    pts[n / 2] = Affine<F>::inf();
    // the scale loop against independently computed scalars
    const Fr x = rand_fr(), c = rand_fr();
    const uint64_t first = ((uint64_t)1 << 32) + 5;
    std::vector<Affine<F>> out(n);
    host_scale_powers<F>((const uint8_t *)pts.data(), n, first, x, c, (uint8_t *)out.data());
    for (int i = 0; i < n; i++) {
        const Fr k = Fr::from_mont(Fr::mul(Fr::pow_u64(x, first + i), c));
        EXPECT(same(out[i], Xyzz<F>::mul_scalar(Xyzz<F>::from_affine(pts[i]), k.v).to_affine()), name);
    }
    EXPECT(out[n / 2].is_inf(), "infinity stays");
    // the two multiplications the kernels use against the generic one
    for (int i = 0; i < n; i++) {
        if (pts[i].is_inf()) continue;
        const Fr km = rand_fr(), k = Fr::from_mont(km);
        const Affine<F> want = Xyzz<F>::mul_scalar(Xyzz<F>::from_affine(pts[i]), k.v).to_affine();
        EXPECT(same(mul_affine_k256<F>(pts[i], k256_of_mont(km)).to_affine(), want), "mul_affine_k256");
        EXPECT(same(mul_naf<F>(pts[i], naf_recode(k)).to_affine(), want), "mul_naf");
    }
    // the predicates
    PointsCount cnt;
    host_points_validate<F>((const uint8_t *)pts.data(), n, &cnt);
    EXPECT(cnt.infinity == 1 && !cnt.range && !cnt.curve && !cnt.subgroup && cnt.first_bad == (uint64_t)(n / 2), "validate: one infinity");
    Affine<F> bad = pts[0];
    bad.y = pts[1].y;
    EXPECT(host_point_class<F>(bad) == PT_CURVE, "validate: off the curve");
    bad = pts[0];
    memset(&bad.y, 0xff, sizeof bad.y);
    EXPECT(host_point_class<F>(bad) == PT_RANGE, "validate: out of range");
    EXPECT(host_point_class<F>(pts[0]) == PT_GOOD, "validate: good");
    // r walked in non-adjacent form: the point at infinity for every point of the group
    const NafDigits r = naf_recode(r_as_limbs());
    for (int i = 0; i < 8; i++) EXPECT(mul_naf<F>(pts[i], r).is_inf(), "[r] P");
}

// a point on the twist outside the order-r subgroup: the first x = (t, 1) whose right-hand side has a square root (p = 3 mod 4: the
// complex method), as the validation must see it
static bool fq2_sqrt(const Fq2 &a, Fq2 *out) {
    // a^((q^2 + 7) / 16)-style shortcuts need tower constants; the exponentiation a^((q - 3) / 4) of the complex method needs only Fq2::mul
    uint32_t e[8];      // (q - 3) / 4
    { uint64_t br = 3; uint32_t t[8]; for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)FqParams::p(i) - br; t[i] = (uint32_t)d; br = (d >> 63) & 1; }
      for (int i = 0; i < 8; i++) e[i] = t[i] >> 2 | (i < 7 ? t[i + 1] << 30 : 0); }
    Fq2 a1 = Fq2::one(), base = a;
    for (int i = 0; i < 256; i++) { if ((e[i >> 5] >> (i & 31)) & 1) a1 = Fq2::mul(a1, base); base = Fq2::sqr(base); }
    const Fq2 x0 = Fq2::mul(a1, a), alpha = Fq2::mul(a1, x0);
    const Fq2 minus_one = Fq2::neg(Fq2::one());
    Fq2 x;
    if (alpha == minus_one) { x = Fq2{Fq::neg(x0.c1), x0.c0}; }      // i * x0
    else {
        uint32_t h[8];      // (q - 1) / 2
        { uint32_t t[8]; for (int i = 0; i < 8; i++) t[i] = FqParams::p(i); t[0] -= 1; for (int i = 0; i < 8; i++) h[i] = t[i] >> 1 | (i < 7 ? t[i + 1] << 31 : 0); }
        Fq2 b = Fq2::one(), bb = Fq2::add(alpha, Fq2::one());
        for (int i = 0; i < 256; i++) { if ((h[i >> 5] >> (i & 31)) & 1) b = Fq2::mul(b, bb); bb = Fq2::sqr(bb); }
        x = Fq2::mul(b, x0);
    }
    *out = x;
    return Fq2::sqr(x) == a;
}

int main() {
    check_group<Fq>("g1 scale", 200);
    check_group<Fq2>("g2 scale", 100);
    const NafDigits r = naf_recode(r_as_limbs());
    int found = 0;
    for (uint64_t t = 1; t < 64 && found < 4; t++) {
        G2Affine p;
        p.x = Fq2{Fq::from_u64(t), Fq::one()};
        const Fq2 rhs = Fq2::add(Fq2::mul(Fq2::sqr(p.x), p.x), CurveOf<Fq2>::b());
        if (!fq2_sqrt(rhs, &p.y)) continue;
        found++;
        EXPECT(point_class_on_curve<Fq2>(p) == PT_GOOD, "a constructed point is on the twist");
        const bool inf_naf = mul_naf<Fq2>(p, r).is_inf(), inf_ref = Xyzz<Fq2>::mul_scalar(Xyzz<Fq2>::from_affine(p), r_as_limbs().v).is_inf();
        EXPECT(inf_naf == inf_ref, "mul_naf<Fq2> of r against mul_scalar");
        EXPECT(!inf_ref, "a random point of the twist is outside the subgroup");
        EXPECT(host_point_class<Fq2>(p) == PT_SUBGROUP, "validate: outside the subgroup");
    }
    EXPECT(found == 4, "points on the twist were found");
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
