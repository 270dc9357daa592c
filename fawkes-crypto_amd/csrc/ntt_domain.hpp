// The evaluation domain of a transform size and its tables (ntt.hip builds and owns them: fk_ctx::domains), and the quotient over rows of it: what batch_prove.hip takes from ntt.hip.
#pragma once
#include "common.hpp"

namespace fk {

struct ScaleTable {          // value(i) = lo[i & (2^L - 1)] * hi[i >> L]
    Fr *lo = nullptr, *hi = nullptr;
    Fr *full = nullptr;      // the products themselves (the quotient's two post-scale tables, memory permitting): one product per element instead of two
};

struct NttDomain {
    uint32_t log_n = 0, L = 0, maxdeg = 0;
    std::vector<uint32_t> degs;
    Fr omega, omega_inv, minv, zinv;
    Fr *tw_lo[2] = {nullptr, nullptr}, *tw_hi[2] = {nullptr, nullptr};   // [0] forward, [1] inverse
    Fr *pq[2] = {nullptr, nullptr};                                       // omega_Rmax^e, e < Rmax/2
    ScaleTable t_g, t_ginv_minv, t_g_minv, t_ginv_minv_zinv;
    // single-level inter-pass twiddles: tw_full[dir][pass][k * r] = w^((k * r) << (log_n - lgp - deg)); one product per
    // element instead of two (lo * hi, then the element).  nullptr: fall back to the two-level tables.
    std::vector<Fr *> tw_full[2];
    std::map<uint64_t, ScaleTable> dist_post;   // distributed quotient: (omega_m^-rank)^k tables, key = log_w << 32 | rank
    std::vector<void *> allocs;
};

// ntt.hip: the context's domain of 2^log_n points, built on first use
int get_domain(fk_ctx *ctx, uint32_t log_n, NttDomain **out);
// ntt.hip: the quotients of `proofs` rows of 2^d->log_n elements (a, b, c zero behind their rows; s1, s2: proofs << log_n elements of scratch each)
int quotient_rows(fk_ctx *ctx, NttDomain *d, Fr *d_a, Fr *d_b, Fr *d_c, uint32_t proofs, Fr *s1, Fr *s2, Fr *d_h);

}  // namespace fk
