// BN254 G1 / G2 group arithmetic, generic over the coordinate field (Fq or Fq2).
//
// Affine points use the raw layout fawkes-crypto exchanges with bellman (`into_raw_uncompressed_le`,
// backend/bellman_groth16/group.rs:57-66 and :97-103): Montgomery LE x || y, and the all-zero buffer is
// the point at infinity (group.rs:55,71-72,89-93).  Accumulators are XYZZ (x = X/ZZ, y = Y/ZZZ,
// ZZ^3 = ZZZ^2; infinity <=> ZZ == 0): a mixed addition costs 8M+2S instead of Jacobian's 7M+4S and
// needs no inversion.  Any correct group law yields the same affine result, so the 256 proof bytes
// are independent of the coordinate system.
#pragma once
#include "field.hpp"

namespace fk {

template <class F>
struct alignas(16) Affine {
    F x, y;
    FK_HD bool is_inf() const { return x.is_zero() && y.is_zero(); }
    static FK_HD Affine inf() { return Affine{F::zero(), F::zero()}; }
};

template <class F>
struct alignas(16) Xyzz {
    F x, y, zz, zzz;

    static FK_HD Xyzz inf() { return Xyzz{F::zero(), F::zero(), F::zero(), F::zero()}; }
    FK_HD bool is_inf() const { return zz.is_zero(); }
    static FK_HD Xyzz from_affine(const Affine<F> &p) {
        if (p.is_inf()) return inf();
        return Xyzz{p.x, p.y, F::one(), F::one()};
    }

    // 2 * (affine p), p not infinity (mdbl-2008-s-1)
    static FK_HD Xyzz dbl_affine(const Affine<F> &p) {
        F u = F::dbl(p.y);
        F v = F::sqr(u);
        F w = F::mul(u, v);
        F s = F::mul(p.x, v);
        F xx = F::sqr(p.x);
        F m = F::add(F::dbl(xx), xx);
        Xyzz r;
        r.x = F::sub(F::sqr(m), F::dbl(s));
        r.y = F::sub(F::mul(m, F::sub(s, r.x)), F::mul(w, p.y));
        r.zz = v;
        r.zzz = w;
        return r;
    }

    // dbl-2008-s-1
    static FK_HD Xyzz dbl(const Xyzz &p) {
        if (p.is_inf()) return p;
        F u = F::dbl(p.y);
        F v = F::sqr(u);
        F w = F::mul(u, v);
        F s = F::mul(p.x, v);
        F xx = F::sqr(p.x);
        F m = F::add(F::dbl(xx), xx);
        Xyzz r;
        r.x = F::sub(F::sqr(m), F::dbl(s));
        r.y = F::sub(F::mul(m, F::sub(s, r.x)), F::mul(w, p.y));
        r.zz = F::mul(v, p.zz);
        r.zzz = F::mul(w, p.zzz);
        return r;
    }

    // acc += q (affine), madd-2008-s with the exceptional cases handled
    FK_HD void add_mixed(const Affine<F> &q) {
        if (q.is_inf()) return;
        add_mixed_nz(q);
    }
    // the same for a q known not to be the point at infinity
    FK_HD void add_mixed_nz(const Affine<F> &q) {
        if (is_inf()) { x = q.x; y = q.y; zz = F::one(); zzz = F::one(); return; }
        // the ten multiplications form five independent pairs -> four dual-chain products (F::mul2) and one fused difference of two (F::mulsub)
        F u2, s2;
        F::mul2(q.x, zz, q.y, zzz, u2, s2);
        F p, r;
        F::sub2(u2, x, s2, y, p, r);                 // independent differences: one dual-chain operation
        if (p.is_zero()) {
            if (r.is_zero()) *this = dbl_affine(q); else *this = inf();
            return;
        }
        F pp, rr;
        F::sqr2(p, r, pp, rr);
        F ppp, q_;
        F::mul2(p, pp, x, pp, ppp, q_);
        F q2, t1;
        F::addsub2(q_, q_, rr, ppp, q2, t1);         // q2 = 2 q, t1 = rr - ppp
        F x3 = F::sub(t1, q2);
        y = F::mulsub(r, F::sub(q_, x3), y, ppp);      // r (q - x3) - y ppp: one reduction in G1 on the device (field.hpp)
        x = x3;
        F::mul2(zz, pp, zzz, ppp, zz, zzz);
    }

    // acc += q (XYZZ), add-2008-s with the exceptional cases handled
    FK_HD void add(const Xyzz &q) {
        if (q.is_inf()) return;
        if (is_inf()) { *this = q; return; }
        F u1 = F::mul(x, q.zz);
        F u2 = F::mul(q.x, zz);
        F s1 = F::mul(y, q.zzz);
        F s2 = F::mul(q.y, zzz);
        F p = F::sub(u2, u1);
        F r = F::sub(s2, s1);
        if (p.is_zero()) {
            if (r.is_zero()) *this = dbl(*this); else *this = inf();
            return;
        }
        F pp = F::sqr(p);
        F ppp = F::mul(p, pp);
        F q_ = F::mul(u1, pp);
        F x3 = F::sub(F::sub(F::sqr(r), ppp), F::dbl(q_));
        y = F::sub(F::mul(r, F::sub(q_, x3)), F::mul(s1, ppp));
        x = x3;
        zz = F::mul(F::mul(zz, q.zz), pp);
        zzz = F::mul(F::mul(zzz, q.zzz), ppp);
    }

    FK_HD Affine<F> to_affine() const {  // one inversion: 1/(zz*zzz) -> 1/zz, 1/zzz
        if (is_inf()) return Affine<F>::inf();
        F t = F::inv(F::mul(zz, zzz));
        F izz = F::mul(t, zzz);
        F izzz = F::mul(t, zz);
        return Affine<F>{F::mul(x, izz), F::mul(y, izzz)};
    }

    // k * p, k canonical 8 x u32 LE (the proof's assembly only: groth16_assemble)
    static FK_HD Xyzz mul_scalar(const Xyzz &p, const uint32_t k[8]) {
        Xyzz acc = inf();
        for (int i = 255; i >= 0; i--) {
            acc = dbl(acc);
            if ((k[i >> 5] >> (i & 31)) & 1) acc.add(p);
        }
        return acc;
    }

    // k * p for an affine p and a k of at most 128 bits, k = hi 2^64 + lo: `nbits` double-and-add steps from bit nbits - 1 down, mixed
    // additions.  The scalar is walked by shifting it left -- no run-time index into a register array, so nothing goes to scratch.
    static FK_HD Xyzz mul_affine_bits(const Affine<F> &p, uint64_t lo, uint64_t hi, int nbits) {
        Xyzz acc = inf();
        if (p.is_inf()) return acc;
        for (int s = 128 - nbits; s > 0; s--) { hi = hi << 1 | lo >> 63; lo <<= 1; }
        for (int i = 0; i < nbits; i++) {
            acc = dbl(acc);
            if (hi >> 63) acc.add_mixed_nz(p);
            hi = hi << 1 | lo >> 63; lo <<= 1;
        }
        return acc;
    }
};

template <class F>
static FK_HD Affine<F> affine_neg_if(const Affine<F> &p, bool neg) {
    // -(x, y) = (x, -y); infinity (0,0) maps to itself because neg(0) == 0
    return neg ? Affine<F>{p.x, F::neg(p.y)} : p;
}

using G1Affine = Affine<Fq>;
using G2Affine = Affine<Fq2>;
using G1Xyzz = Xyzz<Fq>;
using G2Xyzz = Xyzz<Fq2>;

// k * p on the host for a Montgomery k, affine in and out: the vk points of a setup, the deltas of a ceremony contribution, and the
// reference the scale kernel of ceremony.hip is compared with
template <class F>
static inline Affine<F> host_mul(const Affine<F> &p, const Fr &k_mont) {
    const Fr k = Fr::from_mont(k_mont);
    return Xyzz<F>::mul_scalar(Xyzz<F>::from_affine(p), k.v).to_affine();
}

// The key's five points that enter every proof.
struct AssembleKey { G1Affine alpha_g1, beta_g1, delta_g1; G2Affine beta_g2, delta_g2; };

// The Groth16 proof from the five sums H, L, A_q, B1 (G1) and B2 (G2) and r, s (Montgomery form):
//   A = alpha + A_q + r*delta1 ; B = beta2 + B2 + s*delta2 ;
//   C = H + L + s*A_q + r*B1 + s*alpha + r*beta1 + (r s)*delta1   
// out: fawkes Borsh, A.x A.y B.x.c0 B.x.c1 B.y.c0 B.y.c1 C.x C.y as canonical LE words, infinity = zeros (Fq::from_mont(0) == 0).
// The one place the proof bytes come from: fk_prove_assemble on the host, batch_assemble_kernel one proof per lane.
static FK_HD void groth16_assemble(const AssembleKey &key, const G1Xyzz &H, const G1Xyzz &L, const G1Xyzz &A, const G1Xyzz &B1, const G2Xyzz &B2,
                                   const Fr &rm, const Fr &sm, Fq out[8]) {
    const Fr rc = Fr::from_mont(rm), sc = Fr::from_mont(sm), rsc = Fr::from_mont(Fr::mul(rm, sm));
    const G1Xyzz d1 = G1Xyzz::from_affine(key.delta_g1), a1 = G1Xyzz::from_affine(key.alpha_g1), b1 = G1Xyzz::from_affine(key.beta_g1);
    const G2Xyzz d2 = G2Xyzz::from_affine(key.delta_g2);
    G1Xyzz gA = G1Xyzz::mul_scalar(d1, rc.v); gA.add_mixed(key.alpha_g1); gA.add(A);
    G2Xyzz gB = G2Xyzz::mul_scalar(d2, sc.v); gB.add_mixed(key.beta_g2); gB.add(B2);
    G1Xyzz gC = G1Xyzz::mul_scalar(d1, rsc.v);
    gC.add(G1Xyzz::mul_scalar(a1, sc.v));
    gC.add(G1Xyzz::mul_scalar(b1, rc.v));
    gC.add(G1Xyzz::mul_scalar(A, sc.v));
    gC.add(G1Xyzz::mul_scalar(B1, rc.v));
    gC.add(H); gC.add(L);
    const G1Affine pa = gA.to_affine(), pc = gC.to_affine();
    const G2Affine pb = gB.to_affine();
    out[0] = Fq::from_mont(pa.x); out[1] = Fq::from_mont(pa.y);
    out[2] = Fq::from_mont(pb.x.c0); out[3] = Fq::from_mont(pb.x.c1); out[4] = Fq::from_mont(pb.y.c0); out[5] = Fq::from_mont(pb.y.c1);
    out[6] = Fq::from_mont(pc.x); out[7] = Fq::from_mont(pc.y);
}

}  // namespace fk
