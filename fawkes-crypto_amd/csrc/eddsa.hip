// JubJub over BN254 Fr and the EdDSA-Poseidon signature on the device (native/ecc.rs, native/eddsaposeidon.rs, engines/bn256/mod.rs:28-75):
// batch scalar multiplication, subgroup decompression, signature verification and the point half of signing -- one item per lane.
//
// Curve: -x^2 + y^2 = 1 + d x^2 y^2, d = -168696/168700.  d is a non-residue and -1 a residue mod r, so the addition law is complete: no
// lane ever needs an exceptional-case branch and 1 - d x^2 is never zero.  Points are extended (X : Y : T : Z), T = X Y / Z; an affine
// operand is held as (y - x, y + x, 2 d x y), which makes the unified addition 7 products; a doubling is 4 squarings + 4 products.
// Every multiplication is double-and-add, most significant bit first, with the same trip count in every lane; the per-bit addition is
// computed always and SELECTED limb by limb (wave-uniform scalars -- the constant Fs of the subgroup check -- branch instead: no lane
// diverges).  Scalars are walked by shifting their 256-bit image left: no run-time index into a register array, hence no scratch.
// The curve constants, the generator, the bits of Fs and the exponents sit in one small device record (JjConst) that every lane reads
// through the same address (scalar loads), like the Poseidon table.
//
// Products (squarings counted as products), Poseidon at (t, f, p) = (4, 8, 54) = 1250; DESIGN 3.7 has the derivation:
//   inverse       a^(r - 2): 253 squarings + 126 products ....................................................    379
//   square root   a^((t - 1) / 2): 224 + 98; x and b: 2; 27 Tonelli-Shanks rounds: 351 + 27 * 3; the check: 1 ....    757
//   decompress    3 + inverse + root + 3 (the affine operand) + [Fs] P: 250 * 8 + 114 * 7 .......................   3940
//   mul           256 * (8 + 7) + inverse + 2 (+ 2 for a point that is not the generator) ........................   4221
//   verify        2 decompress + Poseidon + 1 + 2 + 251 * (8 + 7 + 7) + 2 ........................................  14657
//   sign          2 * 251 * 15 + 1 + inverse + 4 + Poseidon + 1 ..................................................   9165
#include "poseidon.hpp"
#include <mutex>

namespace fk {

static constexpr uint32_t JJ_THREADS = 64;      // one wave per workgroup: a batch of 4096 spreads over 64 compute units
static constexpr int FS_BITS = 251;             // Fs < 2^251
static constexpr int FR_TWO_ADICITY = 28;       // r - 1 = 2^28 t
static constexpr int TS_W_BITS = 225;           // bits of (t - 1) / 2
static constexpr int FR_BITS = 254;

struct alignas(16) U256 { uint32_t v[8]; };     // a canonical little-endian integer (scalars, Fs elements)

struct JjConst {
    Fr d, d2;                       // d, 2 d
    Fr gx, gy;                      // the generator, affine
    Fr g_ymx, g_ypx, g_t2d;         // ... and as an addition operand
    Fr ts_z;                        // c^t for a non-residue c: generates the 2^28-th roots of unity
    uint32_t fs[8];                 // Fs
    uint32_t e_w[8];                // (t - 1) / 2
    uint32_t e_inv[8];              // r - 2
};

struct Ext { Fr X, Y, T, Z; };
struct Niels { Fr ymx, ypx, t2d; };

namespace jj {

static FK_HD Fr sel(bool c, const Fr &a, const Fr &b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}
static FK_HD Ext sel(bool c, const Ext &a, const Ext &b) { return Ext{sel(c, a.X, b.X), sel(c, a.Y, b.Y), sel(c, a.T, b.T), sel(c, a.Z, b.Z)}; }

// a < b as 256-bit integers: the borrow out of a - b
template <class B>
static FK_HD bool below(const uint32_t *a, B b) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a[i] - b(i) - br; br = (uint32_t)(t >> 63); }
    return br != 0;
}
static FK_HD bool fr_canonical(const Fr &a) { return below(a.v, [](int i) { return FrParams::p(i); }); }

// k -= m << sh if that leaves k >= 0, for sh = top .. 0: k mod m whenever k < m << (top + 1)
static FK_HD void reduce_by(U256 &k, const uint32_t *m, int top) {
    for (int sh = top; sh >= 0; sh--) {
        U256 d; uint32_t br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t mi = sh ? (m[i] << sh) | (i ? m[i - 1] >> (32 - sh) : 0) : m[i];
            const uint64_t t = (uint64_t)k.v[i] - mi - br;
            d.v[i] = (uint32_t)t; br = (uint32_t)(t >> 63);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) k.v[i] = br ? k.v[i] : d.v[i];
    }
}

static FK_HD U256 shl(const U256 &k, int sh) {       // 0 < sh < 32
    U256 r;
#pragma unroll
    for (int i = 7; i >= 0; i--) r.v[i] = (k.v[i] << sh) | (i ? k.v[i - 1] >> (32 - sh) : 0);
    return r;
}
static FK_HD bool take_top_bit(U256 &k) {
    const bool b = (k.v[7] >> 31) != 0;
    k = shl(k, 1);
    return b;
}

// a^e for a wave-uniform exponent of `bits` bits (its top bit set): the branch is the same in every lane
static FK_HD Fr pow_uniform(const Fr &a, const uint32_t *__restrict__ e, int bits) {
    Fr acc = a;
#pragma nounroll
    for (int i = bits - 2; i >= 0; i--) {
        acc = Fr::sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = Fr::mul(acc, a);
    }
    return acc;
}
static FK_HD Fr inv(const Fr &a, const JjConst *__restrict__ c) { return pow_uniform(a, c->e_inv, FR_BITS); }

// Tonelli-Shanks for r - 1 = 2^28 t with a fixed trip count.  x^2 = a b holds throughout; round i brings the order of b down to a divisor
// of 2^(26 - i).  Returns whether a is a square (then root^2 = a); the root of 0 is 0.
static FK_HD bool fr_sqrt(const Fr &a, const JjConst *__restrict__ c, Fr &root) {
    const Fr w = pow_uniform(a, c->e_w, TS_W_BITS);
    Fr x = Fr::mul(a, w), b = Fr::mul(x, w), z = c->ts_z;
    const Fr one = Fr::one();
#pragma nounroll
    for (int i = 0; i < FR_TWO_ADICITY - 1; i++) {
        Fr t = b;
#pragma nounroll
        for (int j = 0; j < FR_TWO_ADICITY - 2 - i; j++) t = Fr::sqr(t);
        const bool m = t != one;
        const Fr z2 = Fr::sqr(z);
        Fr xz, bz;
        Fr::mul2(x, z, b, z2, xz, bz);
        x = sel(m, xz, x); b = sel(m, bz, b); z = z2;
    }
    root = x;
    return Fr::sqr(x) == a;
}

static FK_HD Ext identity() { return Ext{Fr::zero(), Fr::one(), Fr::zero(), Fr::one()}; }
static FK_HD Niels niels_of(const Fr &x, const Fr &y, const Fr &d2) {
    Niels q;
    Fr::addsub2(y, x, y, x, q.ypx, q.ymx);
    q.t2d = Fr::mul(Fr::mul(x, y), d2);
    return q;
}

// ecc.rs:282-307 (a = -1): A = X^2, B = Y^2, C = 2 Z^2, E = (X + Y)^2 - A - B, G = B - A, F = G - C, H = -(A + B)
static FK_HD Ext dbl(const Ext &p) {
    Fr A, B, zz, S;
    const Fr xy = Fr::add(p.X, p.Y);
    Fr::sqr2(p.X, p.Y, A, B);
    Fr::sqr2(p.Z, xy, zz, S);
    const Fr C = Fr::dbl(zz);
    Fr apb, G, E, F;
    Fr::addsub2(A, B, B, A, apb, G);
    Fr::sub2(S, apb, G, C, E, F);
    const Fr H = Fr::neg(apb);
    Ext r;
    Fr::mul2(E, F, G, H, r.X, r.Y);
    Fr::mul2(E, H, F, G, r.T, r.Z);
    return r;
}

// ecc.rs:309-333 with an affine second operand: A = (Y1 - X1)(y2 - x2), B = (Y1 + X1)(y2 + x2), C = T1 2 d x2 y2, D = 2 Z1
static FK_HD Ext add(const Ext &p, const Niels &q) {
    Fr ypx, ymx, A, B;
    Fr::addsub2(p.Y, p.X, p.Y, p.X, ypx, ymx);
    Fr::mul2(ymx, q.ymx, ypx, q.ypx, A, B);
    const Fr C = Fr::mul(p.T, q.t2d);
    const Fr D = Fr::dbl(p.Z);
    Fr H, E, G, F;
    Fr::addsub2(B, A, B, A, H, E);
    Fr::addsub2(D, C, D, C, G, F);
    Ext r;
    Fr::mul2(E, F, G, H, r.X, r.Y);
    Fr::mul2(E, H, F, G, r.T, r.Z);
    return r;
}

// [k] q, k < 2^NBITS, one scalar per lane (ecc.rs:339-352)
template <int NBITS>
static FK_HD Ext mul(const Niels &q, U256 k) {
    if constexpr (NBITS < 256) k = shl(k, 256 - NBITS);
    Ext acc = identity();
#pragma nounroll
    for (int i = 0; i < NBITS; i++) {
        acc = dbl(acc);
        const bool bit = take_top_bit(k);
        acc = sel(bit, add(acc, q), acc);
    }
    return acc;
}

// [k1] q1 + [k2] q2 over one chain of doublings
template <int NBITS>
static FK_HD Ext mul2(const Niels &q1, U256 k1, const Niels &q2, U256 k2) {
    if constexpr (NBITS < 256) { k1 = shl(k1, 256 - NBITS); k2 = shl(k2, 256 - NBITS); }
    Ext acc = identity();
#pragma nounroll
    for (int i = 0; i < NBITS; i++) {
        acc = dbl(acc);
        const bool b1 = take_top_bit(k1);
        acc = sel(b1, add(acc, q1), acc);
        const bool b2 = take_top_bit(k2);
        acc = sel(b2, add(acc, q2), acc);
    }
    return acc;
}

// [Fs] (x, y): the bits of Fs are the same in every lane
static FK_HD Ext mul_fs(const Fr &x, const Fr &y, const JjConst *__restrict__ c) {
    const Niels q = niels_of(x, y, c->d2);
    Ext acc{x, y, Fr::mul(x, y), Fr::one()};
#pragma nounroll
    for (int i = FS_BITS - 2; i >= 0; i--) {
        acc = dbl(acc);
        if ((c->fs[i >> 5] >> (i & 31)) & 1) acc = add(acc, q);
    }
    return acc;
}

// ecc.rs:71-92.  y = sqrt((x^2 + 1) / (1 - d x^2)); [Fs] (x, y) must have X = 0, and is then (0 : Z : 0 : Z) or (0 : -Z : 0 : Z): the second
// means (x, y) is a subgroup point plus the point of order two, and (x, -y) is the subgroup point.  Either root gives the same answer.
static FK_HD bool decompress(const Fr &x, const JjConst *__restrict__ c, Fr &y_out) {
    const Fr x2 = Fr::sqr(x);
    const Fr num = Fr::add(x2, Fr::one()), den = Fr::sub(Fr::one(), Fr::mul(c->d, x2));
    const Fr a = Fr::mul(num, inv(den, c));
    Fr y;
    const bool has_root = fr_sqrt(a, c, y);
    const Ext l = mul_fs(x, y, c);
    y_out = sel(l.Y == l.Z, y, Fr::neg(y));
    return has_root && l.X.is_zero();
}

// eddsaposeidon.rs:53-79 behind the hash: both decompressions, then [s] G - [h] A == R by cross-multiplication (ecc.rs:50-54)
static FK_HD bool verify_core(const JjConst *__restrict__ c, const U256 &s, const Fr &r, const Fr &a, const U256 &h) {
    Fr xs = a, ya = Fr::zero(), yr = Fr::zero();
    bool ok = true;
#pragma nounroll
    for (int k = 0; k < 2; k++) {       // a loop, not two copies of the code
        Fr y;
        ok = decompress(xs, c, y) && ok;
        if (k == 0) { ya = y; xs = r; } else yr = y;
    }
    const Niels minus_a = niels_of(Fr::neg(a), ya, c->d2);
    const Niels g{c->g_ymx, c->g_ypx, c->g_t2d};
    const Ext p = mul2<FS_BITS>(minus_a, h, g, s);
    Fr u, v;
    Fr::mul2(r, p.Z, yr, p.Z, u, v);
    return ok && p.X == u && p.Y == v;
}

static FK_HD U256 canonical_of(const Fr &a) {
    const Fr t = Fr::from_mont(a);
    U256 k;
#pragma unroll
    for (int i = 0; i < 8; i++) k.v[i] = t.v[i];
    return k;
}
// to_other_reduced: r < 8 Fs
static FK_HD U256 hash_scalar(const Fr &h, const JjConst *__restrict__ c) { U256 k = canonical_of(h); reduce_by(k, c->fs, 2); return k; }

}  // namespace jj

// ------------------------------------------------------------------------------------------ kernels
// points == nullptr: the generator
__global__ __launch_bounds__(JJ_THREADS) void jubjub_mul_kernel(const JjConst *__restrict__ c, const Fr *__restrict__ points, const U256 *__restrict__ scalars, size_t n,
                                                               Fr *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Niels q = points ? jj::niels_of(points[2 * i], points[2 * i + 1], c->d2) : Niels{c->g_ymx, c->g_ypx, c->g_t2d};
    const Ext p = jj::mul<256>(q, scalars[i]);
    const Fr zi = jj::inv(p.Z, c);
    Fr::mul2(p.X, zi, p.Y, zi, out[2 * i], out[2 * i + 1]);
}

__global__ __launch_bounds__(JJ_THREADS) void jubjub_decompress_kernel(const JjConst *__restrict__ c, const Fr *__restrict__ x, size_t n, Fr *__restrict__ y,
                                                                      uint8_t *__restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr yy;
    const bool good = jj::decompress(x[i], c, yy);
    y[i] = jj::sel(good, yy, Fr::zero());
    ok[i] = good ? 1 : 0;
}

// a row whose s is not below Fs, or whose r / a / m image is not below the modulus, is rejected (its lane computes on zeros)
__global__ __launch_bounds__(JJ_THREADS) void eddsa_verify_kernel(const JjConst *__restrict__ c, const Fr *__restrict__ tab, uint32_t f, uint32_t p,
                                                                 const U256 *__restrict__ s, const Fr *__restrict__ r, const Fr *__restrict__ a, const Fr *__restrict__ m,
                                                                 size_t n, uint8_t *__restrict__ accept) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    U256 si = s[i];
    Fr ri = r[i], ai = a[i], mi = m[i];
    const uint32_t *fs = c->fs;
    const bool valid = jj::below(si.v, [fs](int j) { return fs[j]; }) && jj::fr_canonical(ri) && jj::fr_canonical(ai) && jj::fr_canonical(mi);
    const Fr zero = Fr::zero();
    ri = jj::sel(valid, ri, zero); ai = jj::sel(valid, ai, zero); mi = jj::sel(valid, mi, zero);
#pragma unroll
    for (int j = 0; j < 8; j++) si.v[j] = valid ? si.v[j] : 0;
    Fr st[4] = {ri, ai, mi, zero};
    PoseidonPerm<4>::run(st, tab, f, p);
    const U256 h = jj::hash_scalar(st[0], c);
    const bool ok = jj::verify_core(c, si, ri, ai, h);
    accept[i] = (valid && ok) ? 1 : 0;
}

// the point half of eddsaposeidon.rs:42-53: R = [rho] G, A = [sk] G, their affine x through ONE inversion, h = poseidon([r_x, a_x, m]) mod Fs
__global__ __launch_bounds__(JJ_THREADS) void eddsa_sign_points_kernel(const JjConst *__restrict__ c, const Fr *__restrict__ tab, uint32_t f, uint32_t p,
                                                                      const U256 *__restrict__ sk, const U256 *__restrict__ rho, const Fr *__restrict__ m, size_t n,
                                                                      Fr *__restrict__ r_x, Fr *__restrict__ a_x, U256 *__restrict__ h) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Niels g{c->g_ymx, c->g_ypx, c->g_t2d};
    U256 k = rho[i];
    Ext pr = jj::identity(), pa = jj::identity();
#pragma nounroll
    for (int j = 0; j < 2; j++) {
        const Ext q = jj::mul<FS_BITS>(g, k);
        if (j == 0) { pr = q; k = sk[i]; } else pa = q;
    }
    const Fr zi = jj::inv(Fr::mul(pr.Z, pa.Z), c);
    Fr u, v;
    Fr::mul2(pr.X, pa.Z, pa.X, pr.Z, u, v);
    Fr rx, ax;
    Fr::mul2(u, zi, v, zi, rx, ax);
    Fr st[4] = {rx, ax, m[i], Fr::zero()};
    PoseidonPerm<4>::run(st, tab, f, p);
    r_x[i] = rx; a_x[i] = ax;
    h[i] = jj::hash_scalar(st[0], c);
}

// ------------------------------------------------------------------------------------------ host: the curve constants, derived once
static void u256_of_fr_modulus(uint32_t out[8]) { for (int i = 0; i < 8; i++) out[i] = FrParams::p(i); }
static void u256_sub_small(uint32_t v[8], uint32_t k) { uint64_t br = k; for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)v[i] - br; v[i] = (uint32_t)t; br = (t >> 63) & 1; } }
static void u256_shr(uint32_t v[8], int sh) { for (int i = 0; i < 8; i++) v[i] = (v[i] >> sh) | (i < 7 ? v[i + 1] << (32 - sh) : 0); }
static int u256_bits(const uint32_t v[8]) { for (int i = 255; i >= 0; i--) if ((v[i >> 5] >> (i & 31)) & 1) return i + 1; return 0; }

// Fs = 2736030358979909402780800718157159386076813972158567259200215660948447373041 (engines/bn256/mod.rs:28-46)
static const uint64_t FS_LIMBS[4] = {0x677297dc392126f1ull, 0xab3eedb83920ee0aull, 0x370a08b6d0302b0bull, 0x060c89ce5c263405ull};

static Fr host_inv(const Fr &a) { return Fr::inv(a); }

// engines/bn256/mod.rs:48-75 and ecc.rs:103-132 (from_scalar_raw of the seedbox "edwards_g"), ecc.rs:213-224 (Montgomery -> Edwards)
static bool jj_derive(JjConst &c, std::string &why) {
    u256_of_fr_modulus(c.e_inv); u256_sub_small(c.e_inv, 2);
    uint32_t t[8];
    u256_of_fr_modulus(t); u256_sub_small(t, 1);
    for (int i = 0; i < FR_TWO_ADICITY; i++) { if (t[0] & 1) { why = "r - 1 is not 2^28 t"; return false; } u256_shr(t, 1); }
    if (!(t[0] & 1)) { why = "r - 1 is not 2^28 t with t odd"; return false; }
    for (int i = 0; i < 8; i++) c.e_w[i] = t[i];
    u256_sub_small(c.e_w, 1); u256_shr(c.e_w, 1);
    if (u256_bits(c.e_w) != TS_W_BITS || u256_bits(c.e_inv) != FR_BITS) { why = "exponent widths"; return false; }
    for (int i = 0; i < 4; i++) { c.fs[2 * i] = (uint32_t)FS_LIMBS[i]; c.fs[2 * i + 1] = (uint32_t)(FS_LIMBS[i] >> 32); }
    if (u256_bits(c.fs) != FS_BITS) { why = "Fs width"; return false; }
    const Fr one = Fr::one(), minus_one = Fr::neg(one);
    c.ts_z = Fr::zero();
    for (uint64_t cand = 2; cand < 64; cand++) {         // the first non-residue
        Fr z = Fr::pow(Fr::from_u64(cand), t), top = z;
        for (int i = 0; i < FR_TWO_ADICITY - 1; i++) top = Fr::sqr(top);
        if (top == minus_one) { c.ts_z = z; break; }
    }
    if (c.ts_z.is_zero()) { why = "no small non-residue"; return false; }
    c.d = Fr::neg(Fr::mul(Fr::from_u64(168696), host_inv(Fr::from_u64(168700))));
    c.d2 = Fr::dbl(c.d);
    const Fr opd = host_inv(Fr::add(one, c.d));
    const Fr ma = Fr::mul(Fr::dbl(Fr::sub(one, c.d)), opd), mb = Fr::neg(Fr::mul(Fr::from_u64(4), opd)), mu = Fr::from_u64(337401);
    const Fr mb_inv = host_inv(mb);
    auto gfun = [&](const Fr &x) { return Fr::mul(Fr::add(Fr::mul(Fr::sqr(x), Fr::add(x, ma)), x), mb_inv); };
    const uint8_t salt[] = "edwards_g";
    Seedbox sb(salt, sizeof salt - 1);
    const Fr ts = sb.gen_fr();
    const Fr t2g1 = Fr::mul(Fr::sqr(ts), mu);
    const Fr x2 = Fr::mul(Fr::neg(host_inv(ma)), Fr::add(one, host_inv(t2g1)));
    Fr mx = x2, y;
    if (!jj::fr_sqrt(gfun(mx), &c, y)) {
        mx = Fr::mul(x2, t2g1);
        if (!jj::fr_sqrt(gfun(mx), &c, y)) { why = "from_scalar_raw: neither candidate is on the curve"; return false; }
    }
    if (Fr::from_mont(Fr::mul(y, ts)).v[0] & 1) y = Fr::neg(y);
    if (mx.is_zero() || y.is_zero()) { why = "from_scalar_raw: exceptional point"; return false; }
    const Fr ex = Fr::mul(mx, host_inv(y)), ey = Fr::mul(Fr::sub(mx, one), host_inv(Fr::add(mx, one)));
    Ext p{ex, ey, Fr::mul(ex, ey), one};
    for (int i = 0; i < 3; i++) p = jj::dbl(p);          // the cofactor
    const Fr zi = host_inv(p.Z);
    c.gx = Fr::mul(p.X, zi); c.gy = Fr::mul(p.Y, zi);
    const Niels g = jj::niels_of(c.gx, c.gy, c.d2);
    c.g_ymx = g.ymx; c.g_ypx = g.ypx; c.g_t2d = g.t2d;
    // on the curve, in the subgroup
    const Fr xx = Fr::sqr(c.gx), yy = Fr::sqr(c.gy);
    if (Fr::sub(yy, xx) != Fr::add(one, Fr::mul(c.d, Fr::mul(xx, yy)))) { why = "the generator is not on the curve"; return false; }
    const Ext l = jj::mul_fs(c.gx, c.gy, &c);
    if (!l.X.is_zero() || l.Y != l.Z) { why = "the generator is not in the prime subgroup"; return false; }
    return true;
}

static const JjConst *jj_consts(std::string &why) {
    static JjConst c; static bool ok = false; static std::string err; static std::once_flag once;
    std::call_once(once, [] { ok = jj_derive(c, err); });
    if (!ok) { why = "jubjub: " + err; return nullptr; }
    return &c;
}

// ------------------------------------------------------------------------------------------ host: Blake2s-256 (RFC 7693), one 64-byte block, 8-byte personalisation
static inline uint32_t ror32(uint32_t v, unsigned n) { return (v >> n) | (v << (32 - n)); }

static void blake2s_256_one_block(const uint8_t msg[64], const uint8_t person[8], uint8_t out[32]) {
    static const uint32_t IV[8] = {0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19};
    static const uint8_t SIGMA[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    auto le32 = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; };
    uint32_t h[8], mw[16], v[16];
    for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= 0x01010020;                              // digest 32 bytes, no key, fanout 1, depth 1
    h[6] ^= le32(person); h[7] ^= le32(person + 4);
    for (int i = 0; i < 16; i++) mw[i] = le32(msg + 4 * i);
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= 64;                                     // bytes so far; v[13]: the high word of the counter is zero
    v[14] = ~v[14];                                  // the last block
    auto G = [&](int a, int b, int cc, int d, uint32_t x, uint32_t y) {
        v[a] += v[b] + x; v[d] = ror32(v[d] ^ v[a], 16);
        v[cc] += v[d]; v[b] = ror32(v[b] ^ v[cc], 12);
        v[a] += v[b] + y; v[d] = ror32(v[d] ^ v[a], 8);
        v[cc] += v[d]; v[b] = ror32(v[b] ^ v[cc], 7);
    };
    for (int r = 0; r < 10; r++) {
        const uint8_t *s = SIGMA[r];
        G(0, 4, 8, 12, mw[s[0]], mw[s[1]]); G(1, 5, 9, 13, mw[s[2]], mw[s[3]]); G(2, 6, 10, 14, mw[s[4]], mw[s[5]]); G(3, 7, 11, 15, mw[s[6]], mw[s[7]]);
        G(0, 5, 10, 15, mw[s[8]], mw[s[9]]); G(1, 6, 11, 12, mw[s[10]], mw[s[11]]); G(2, 7, 8, 13, mw[s[12]], mw[s[13]]); G(3, 4, 9, 14, mw[s[14]], mw[s[15]]);
    }
    for (int i = 0; i < 8; i++) { h[i] ^= v[i] ^ v[8 + i]; for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(h[i] >> (8 * b)); }
}

static inline U256 u256_from_limbs(const uint64_t *l) { U256 k; for (int i = 0; i < 4; i++) { k.v[2 * i] = (uint32_t)l[i]; k.v[2 * i + 1] = (uint32_t)(l[i] >> 32); } return k; }
static inline void u256_to_limbs(const U256 &k, uint64_t *l) { for (int i = 0; i < 4; i++) l[i] = (uint64_t)k.v[2 * i] | (uint64_t)k.v[2 * i + 1] << 32; }
static inline bool below_fs(const uint64_t *l) { for (int i = 3; i >= 0; i--) if (l[i] != FS_LIMBS[i]) return l[i] < FS_LIMBS[i]; return false; }

// eddsaposeidon.rs:13-29: Blake2s-256, personalisation "__fawkes", over the 32 little-endian bytes of sk and of m; the digest, read as a
// little-endian integer (< 2^256 < 64 Fs), reduced mod Fs
static void hash_r(const JjConst *c, const uint64_t sk[4], const Fr &m_mont, uint64_t rho[4]) {
    uint8_t msg[64], dig[32];
    const U256 mc = jj::canonical_of(m_mont);
    for (int i = 0; i < 4; i++) for (int b = 0; b < 8; b++) msg[8 * i + b] = (uint8_t)(sk[i] >> (8 * b));
    for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) msg[32 + 4 * i + b] = (uint8_t)(mc.v[i] >> (8 * b));
    blake2s_256_one_block(msg, (const uint8_t *)"__fawkes", dig);
    U256 k;
    for (int i = 0; i < 8; i++) k.v[i] = (uint32_t)dig[4 * i] | (uint32_t)dig[4 * i + 1] << 8 | (uint32_t)dig[4 * i + 2] << 16 | (uint32_t)dig[4 * i + 3] << 24;
    jj::reduce_by(k, c->fs, 5);
    u256_to_limbs(k, rho);
}

// ------------------------------------------------------------------------------------------ host: s = rho + h sk mod Fs (eddsaposeidon.rs:49)
// Plain integers: the 512-bit product h sk is reduced limb by limb -- each of the four outer steps adds the multiple of Fs that clears the
// lowest limb and drops it, which leaves h sk 2^-256 mod Fs; the same step against 2^512 mod Fs takes the factor out again.
struct FsHost { uint64_t n0 = 0, r2[4] = {0, 0, 0, 0}; };

static void fs_add(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {     // a, b < Fs < 2^251
    unsigned __int128 cy = 0; uint64_t s[4];
    for (int i = 0; i < 4; i++) { cy += (unsigned __int128)a[i] + b[i]; s[i] = (uint64_t)cy; cy >>= 64; }
    if (below_fs(s)) { for (int i = 0; i < 4; i++) out[i] = s[i]; return; }
    uint64_t br = 0;
    for (int i = 0; i < 4; i++) { const unsigned __int128 t = (unsigned __int128)s[i] - FS_LIMBS[i] - br; out[i] = (uint64_t)t; br = (uint64_t)(t >> 64) & 1; }
}

static void fs_redc_mul(const FsHost &f, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {    // a b 2^-256 mod Fs
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 cy = 0;
        for (int j = 0; j < 4; j++) { cy += (unsigned __int128)a[j] * b[i] + t[j]; t[j] = (uint64_t)cy; cy >>= 64; }
        cy += t[4]; t[4] = (uint64_t)cy; t[5] = (uint64_t)(cy >> 64);
        const uint64_t q = t[0] * f.n0;
        cy = (unsigned __int128)q * FS_LIMBS[0] + t[0]; cy >>= 64;
        for (int j = 1; j < 4; j++) { cy += (unsigned __int128)q * FS_LIMBS[j] + t[j]; t[j - 1] = (uint64_t)cy; cy >>= 64; }
        cy += t[4]; t[3] = (uint64_t)cy; t[4] = t[5] + (uint64_t)(cy >> 64);
    }
    const uint64_t zero[4] = {0, 0, 0, 0};
    fs_add(t, zero, out);                  // t < 2 Fs: one conditional subtraction
}

static const FsHost &fs_host() {
    static FsHost f; static std::once_flag once;
    std::call_once(once, [] {
        uint64_t x = 1;                                                    // Fs^-1 mod 2^64 by Newton's iteration, negated
        for (int i = 0; i < 6; i++) x *= 2 - FS_LIMBS[0] * x;
        f.n0 = 0 - x;
        uint64_t v[4] = {1, 0, 0, 0};                                      // 2^512 mod Fs by doubling
        for (int i = 0; i < 512; i++) fs_add(v, v, v);
        for (int i = 0; i < 4; i++) f.r2[i] = v[i];
    });
    return f;
}

static void sign_scalar(const uint64_t rho[4], const uint64_t h[4], const uint64_t sk[4], uint64_t s[4]) {
    const FsHost &f = fs_host();
    uint64_t t[4], u[4];
    fs_redc_mul(f, h, sk, t);
    fs_redc_mul(f, t, f.r2, u);
    fs_add(rho, u, s);
}

// ------------------------------------------------------------------------------------------ host drivers
// device image (poseidon.hpp: misc_head): the flag slot, the curve record, the Poseidon table
struct JjDev { const JjConst *c; const Fr *tab; };
static_assert(sizeof(JjConst) <= JJ_CONST_SLOT, "the curve record outgrew its slot");

static int jj_upload(fk_ctx *ctx, const fk_poseidon *h, JjDev *d) {
    std::string why;
    const JjConst *c = jj_consts(why);
    if (!c) FK_SET_ERR(ctx, FK_ERR_UNSUPPORTED, "%s", why.c_str());
    PosDev m; FK_TRY(misc_head(ctx, h, c, sizeof(JjConst), &m));
    *d = JjDev{(const JjConst *)m.curve, m.tab};
    return FK_OK;
}

static inline unsigned jj_blocks(size_t n) { return (unsigned)((n + JJ_THREADS - 1) / JJ_THREADS); }
static constexpr size_t JJ_MAX_BATCH = (size_t)1 << 30;

static int eddsa_args(fk_ctx *ctx, const fk_poseidon *h, size_t n) {
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (h->t != 4) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "eddsa: the signature hashes [r, a, m] with t = 4 parameters (got t = %u)", h->t);
    if (n > JJ_MAX_BATCH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "eddsa: batch too large");
    return FK_OK;
}

static int verify_dev(fk_ctx *ctx, const fk_poseidon *h, const void *d_s, const void *d_r, const void *d_a, const void *d_m, size_t n, void *d_accept) {
    JjDev d; FK_TRY(jj_upload(ctx, h, &d));
    hipLaunchKernelGGL(eddsa_verify_kernel, dim3(jj_blocks(n)), dim3(JJ_THREADS), 0, ctx->stream, d.c, d.tab, h->f, h->p, (const U256 *)d_s, (const Fr *)d_r,
                       (const Fr *)d_a, (const Fr *)d_m, n, (uint8_t *)d_accept);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "eddsa_verify_kernel");
    return FK_OK;
}

static int check_fr_rows(fk_ctx *ctx, const uint64_t *v, size_t rows, const char *what) {
    for (size_t i = 0; i < rows; i++)
        if (!Seedbox::fr_below_modulus(fr_from_limbs(v + 4 * i))) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "%s: element %zu is not below the modulus", what, i);
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_jubjub_params(uint64_t d[4], uint64_t g[8], uint64_t fs[4]) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    std::string why;
    const JjConst *c = jj_consts(why);
    if (!c) { tls_error() = why; return FK_ERR_UNSUPPORTED; }
    if (d) fr_to_limbs(c->d, d);
    if (g) { fr_to_limbs(c->gx, g); fr_to_limbs(c->gy, g + 4); }
    if (fs) for (int i = 0; i < 4; i++) fs[i] = FS_LIMBS[i];
    return FK_OK;
}); }

int fk_eddsa_hash_r(const uint64_t sk[4], const uint64_t m[4], uint64_t rho[4]) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    if (!sk || !m || !rho) { tls_error() = "null argument"; return FK_ERR_BAD_ARG; }
    std::string why;
    const JjConst *c = jj_consts(why);
    if (!c) { tls_error() = why; return FK_ERR_UNSUPPORTED; }
    const Fr mm = fr_from_limbs(m);
    if (!Seedbox::fr_below_modulus(mm)) { tls_error() = "eddsa: m is not below the modulus"; return FK_ERR_BAD_ARG; }
    hash_r(c, sk, mm, rho);
    return FK_OK;
}); }

int fk_jubjub_mul_batch(fk_ctx *ctx, const uint64_t *points, const uint64_t *scalars, size_t n, uint64_t *out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!n) return FK_OK;
    if (!scalars || !out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (n > JJ_MAX_BATCH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "jubjub: batch too large");
    if (points) FK_TRY(check_fr_rows(ctx, points, 2 * n, "jubjub mul: point coordinate"));
    FK_TRY(scratch_claim(ctx, "jubjub mul"));
    const size_t pb = 2 * n * sizeof(Fr), sb = n * sizeof(U256);
    HostStage st{ctx};
    const Fr *d_pts = nullptr; const U256 *d_sc; Fr *d_out;
    if (points) FK_TRY(st.in(ctx->stage_a, points, pb, &d_pts));
    FK_TRY(st.in(ctx->stage_b, scalars, sb, &d_sc)); FK_TRY(st.room(ctx->stage_c, pb, &d_out));
    JjDev d; FK_TRY(jj_upload(ctx, nullptr, &d));
    hipLaunchKernelGGL(jubjub_mul_kernel, dim3(jj_blocks(n)), dim3(JJ_THREADS), 0, ctx->stream, d.c, d_pts, d_sc, n, d_out);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "jubjub_mul_kernel");
    return st.out(out, d_out, pb);
}); }

int fk_jubjub_decompress_batch(fk_ctx *ctx, const uint64_t *x, size_t n, uint64_t *y, uint8_t *ok) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!n) return FK_OK;
    if (!x || !y || !ok) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (n > JJ_MAX_BATCH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "jubjub: batch too large");
    FK_TRY(check_fr_rows(ctx, x, n, "jubjub decompress: x"));
    FK_TRY(scratch_claim(ctx, "jubjub decompress"));
    const size_t xb = n * sizeof(Fr);
    HostStage st{ctx};
    const Fr *d_x; Fr *d_y; uint8_t *d_ok;
    FK_TRY(st.in(ctx->stage_a, x, xb, &d_x)); FK_TRY(st.room(ctx->stage_b, xb, &d_y)); FK_TRY(st.room(ctx->stage_c, n, &d_ok));
    JjDev d; FK_TRY(jj_upload(ctx, nullptr, &d));
    hipLaunchKernelGGL(jubjub_decompress_kernel, dim3(jj_blocks(n)), dim3(JJ_THREADS), 0, ctx->stream, d.c, d_x, n, d_y, d_ok);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "jubjub_decompress_kernel");
    FK_TRY(st.out(y, d_y, xb, false));
    return st.out(ok, d_ok, n);
}); }

int fk_eddsa_sign_batch(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *sk, const uint64_t *m, const uint64_t *rho, size_t n, uint64_t *s, uint64_t *r_x,
                        uint64_t *a_x) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(eddsa_args(ctx, h, n));
    if (!n) return FK_OK;
    if (!sk || !m || !s) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    std::string why;
    const JjConst *c = jj_consts(why);
    if (!c) FK_SET_ERR(ctx, FK_ERR_UNSUPPORTED, "%s", why.c_str());
    FK_TRY(check_fr_rows(ctx, m, n, "eddsa sign: m"));
    for (size_t i = 0; i < n; i++) {
        if (!below_fs(sk + 4 * i)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "eddsa sign: sk %zu is not below Fs", i);
        if (rho && !below_fs(rho + 4 * i)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "eddsa sign: rho %zu is not below Fs", i);
    }
    std::vector<uint64_t> own_rho;
    if (!rho) {
        own_rho.resize(4 * n);
        for (size_t i = 0; i < n; i++) hash_r(c, sk + 4 * i, fr_from_limbs(m + 4 * i), own_rho.data() + 4 * i);
        rho = own_rho.data();
    }
    FK_TRY(scratch_claim(ctx, "eddsa sign"));
    const size_t eb = n * 32;
    HostStage st{ctx};
    const U256 *d_sk, *d_rho; const Fr *d_m;
    FK_TRY(st.use(ctx->stage_a, {eb, eb, eb})); FK_TRY(st.in(sk, eb, &d_sk)); FK_TRY(st.in(rho, eb, &d_rho)); FK_TRY(st.in(m, eb, &d_m));
    FK_TRY(st.use(ctx->stage_b, {eb, eb, eb}));
    Fr *d_rx = st.room<Fr>(eb), *d_ax = st.room<Fr>(eb); U256 *d_h = st.room<U256>(eb);
    JjDev d; FK_TRY(jj_upload(ctx, h, &d));
    hipLaunchKernelGGL(eddsa_sign_points_kernel, dim3(jj_blocks(n)), dim3(JJ_THREADS), 0, ctx->stream, d.c, d.tab, h->f, h->p, d_sk, d_rho, d_m, n, d_rx, d_ax, d_h);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "eddsa_sign_points_kernel");
    std::vector<uint64_t> hs(4 * n);
    if (r_x) FK_TRY(st.out(r_x, d_rx, eb, false));
    if (a_x) FK_TRY(st.out(a_x, d_ax, eb, false));
    FK_TRY(st.out(hs.data(), d_h, eb));
    for (size_t i = 0; i < n; i++) sign_scalar(rho + 4 * i, hs.data() + 4 * i, sk + 4 * i, s + 4 * i);
    return FK_OK;
}); }

int fk_eddsa_verify_batch_dev(fk_ctx *ctx, const fk_poseidon *h, const void *d_s, const void *d_r, const void *d_a, const void *d_m, size_t n, void *d_accept) {
    return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(eddsa_args(ctx, h, n));
    if (!n) return FK_OK;
    if (!d_s || !d_r || !d_a || !d_m || !d_accept) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return verify_dev(ctx, h, d_s, d_r, d_a, d_m, n, d_accept);
}); }

int fk_eddsa_verify_batch(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *s, const uint64_t *r, const uint64_t *a, const uint64_t *m, size_t n, uint8_t *accept) {
    return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(eddsa_args(ctx, h, n));
    if (!n) return FK_OK;
    if (!s || !r || !a || !m || !accept) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_TRY(scratch_claim(ctx, "eddsa verify"));
    const size_t eb = n * 32;
    HostStage st{ctx};
    const void *d_s, *d_r, *d_a, *d_m; uint8_t *d_accept;
    FK_TRY(st.use(ctx->stage_a, {eb, eb, eb, eb}));
    FK_TRY(st.in(s, eb, &d_s)); FK_TRY(st.in(r, eb, &d_r)); FK_TRY(st.in(a, eb, &d_a)); FK_TRY(st.in(m, eb, &d_m));
    FK_TRY(st.room(ctx->stage_b, n, &d_accept));
    FK_TRY(verify_dev(ctx, h, d_s, d_r, d_a, d_m, n, d_accept));
    return st.out(accept, d_accept, n);
}); }

}  // extern "C"
