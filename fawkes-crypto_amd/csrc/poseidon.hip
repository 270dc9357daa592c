// Poseidon over BN254 Fr on the device: batch hashes, the sponge, Merkle trees and Merkle proof roots -- the witness side of the
// rollup workload (native/poseidon.rs: PoseidonParams::new_with_salt, poseidon, poseidon_sponge, poseidon_merkle_proof_root,
// poseidon_merkle_tree_root).  One hash per lane with the state in registers; the round constants and the MDS matrix are the same
// for every lane and are read through wave-uniform indices of a const __restrict__ table (scalar loads).  Rounds are a run-time loop.
//
// Products per hash: (f t + p) * 3 for the S-boxes (x^5 = two squarings and a product) plus (f + p) * t^2 for the mix -- 780 at
// (t, f, p) = (3, 8, 53).  Mix rows: by default each row of the matrix product takes ONE Montgomery reduction per group of up to four
// columns (dot4 / mulsum of field.hpp: canonical operands, sum of k <= 4 products below k p^2, reduced below (1 + 0.19 k) p, one
// conditional subtraction); -DFK_POSEIDON_PLAIN_MIX builds the product-by-product form (same canonical values, hence same bytes).
#include "common.hpp"
#include <string.h>
#include <utility>

struct fk_poseidon {
    uint32_t t = 0, f = 0, p = 0;
    std::vector<fk::Fr> tab;      // (f + p) * t round constants, then t * t matrix entries (row major); Montgomery
};

namespace fk {

static constexpr uint32_t POS_THREADS = 256;
static constexpr uint32_t POS_MAX_T = 8;
static constexpr uint32_t POS_MAX_TREE_DEPTH = 40;  // 2^41 nodes of 32 B do not fit any device

// ------------------------------------------------------------------------------------------ permutation
template <int T>
struct PoseidonPerm {
    static __device__ __forceinline__ void ark(Fr (&s)[T], const Fr *__restrict__ c) {
#pragma unroll
        for (int j = 0; j + 1 < T; j += 2) Fr::add2(s[j], c[j], s[j + 1], c[j + 1], s[j], s[j + 1]);
        if constexpr (T & 1) s[T - 1] = Fr::add(s[T - 1], c[T - 1]);
    }
    static __device__ __forceinline__ Fr sigma1(const Fr &a) { const Fr a2 = Fr::sqr(a); return Fr::mul(Fr::sqr(a2), a); }
    static __device__ __forceinline__ void sigma_all(Fr (&s)[T]) {
#pragma unroll
        for (int j = 0; j + 1 < T; j += 2) {
            Fr x, y;
            Fr::sqr2(s[j], s[j + 1], x, y);
            Fr::sqr2(x, y, x, y);
            Fr::mul2(x, s[j], y, s[j + 1], s[j], s[j + 1]);
        }
        if constexpr (T & 1) s[T - 1] = sigma1(s[T - 1]);
    }
#if defined(FK_POSEIDON_PLAIN_MIX)
    template <int J>
    static __device__ __forceinline__ Fr row_from(const Fr (&s)[T], const Fr *__restrict__ m) {
        if constexpr (T - J >= 2) {
            Fr x, y;
            Fr::mul2(m[J], s[J], m[J + 1], s[J + 1], x, y);
            const Fr d = Fr::add(x, y);
            if constexpr (T - J == 2) return d; else return Fr::add(d, row_from<J + 2>(s, m));
        } else return Fr::mul(m[J], s[J]);
    }
#else
    // one reduction per group of columns: 4 (dot4), 2 (mulsum) or 1 (mul)
    template <int J>
    static __device__ __forceinline__ Fr row_from(const Fr (&s)[T], const Fr *__restrict__ m) {
        if constexpr (T - J >= 4) {
            const Fr d = Fr::dot4(m[J], s[J], m[J + 1], s[J + 1], m[J + 2], s[J + 2], m[J + 3], s[J + 3]);
            if constexpr (T - J == 4) return d; else return Fr::add(d, row_from<J + 4>(s, m));
        } else if constexpr (T - J >= 2) {
#if defined(__HIP_DEVICE_COMPILE__)
            const Fr d = Fr::mulsum_body_asm(m[J], s[J], m[J + 1], s[J + 1]);
#else
            const Fr d = Fr::add(Fr::mul(m[J], s[J]), Fr::mul(m[J + 1], s[J + 1]));      // (host pass of a device function: never called)
#endif
            if constexpr (T - J == 2) return d; else return Fr::add(d, row_from<J + 2>(s, m));
        } else return Fr::mul(m[J], s[J]);
    }
#endif
    // the rows are expanded as a pack, not as a loop: an unrolling the compiler declines would index n[] at run time and put it in scratch
    template <int... I>
    static __device__ __forceinline__ void mix_rows(Fr (&s)[T], const Fr *__restrict__ m, std::integer_sequence<int, I...>) {
        const Fr n[T] = {row_from<0>(s, m + I * T)...};
        ((s[I] = n[I]), ...);
    }
    static __device__ __forceinline__ void mix(Fr (&s)[T], const Fr *__restrict__ m) { mix_rows(s, m, std::make_integer_sequence<int, T>()); }
    // native/poseidon.rs:71-86.  tab: (f + p) * T constants, then the T x T matrix
    static __device__ __forceinline__ void run(Fr (&s)[T], const Fr *__restrict__ tab, uint32_t f, uint32_t p) {
        const uint32_t rounds = f + p, half_f = f >> 1;
        const Fr *__restrict__ m = tab + (size_t)rounds * T;
#pragma nounroll
        for (uint32_t r = 0; r < rounds; r++) {
            ark(s, tab + (size_t)r * T);
            if (r < half_f || r >= half_f + p) sigma_all(s); else s[0] = sigma1(s[0]);
            mix(s, m);
        }
    }
};

template <int T>
__global__ __launch_bounds__(POS_THREADS) void poseidon_hash_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr *__restrict__ in,
                                                                      uint32_t n_inputs, size_t n, Fr *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s[T];
#pragma unroll
    for (int j = 0; j < T; j++) s[j] = (j < T - 1 && (uint32_t)j < n_inputs) ? in[i * n_inputs + j] : Fr::zero();
    PoseidonPerm<T>::run(s, tab, f, p);
    out[i] = s[0];
}

// poseidon.rs:102-110: the stream Fr(len) | message, absorbed T - 1 elements at a time by ADDITION into state[0 .. chunk)
template <int T>
__global__ __launch_bounds__(POS_THREADS) void poseidon_sponge_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr *__restrict__ in,
                                                                        uint64_t len, Fr len_m, size_t n, Fr *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s[T];
#pragma unroll
    for (int j = 0; j < T; j++) s[j] = Fr::zero();
    const Fr *__restrict__ msg = in + i * len;
#pragma nounroll
    for (uint64_t pos = 0; pos < len + 1; pos += T - 1) {
#pragma unroll
        for (int j = 0; j < T - 1; j++) {
            const uint64_t k = pos + j;
            if (k < len + 1) s[j] = Fr::add(s[j], k == 0 ? len_m : msg[k - 1]);
        }
        PoseidonPerm<T>::run(s, tab, f, p);
    }
    out[i] = s[0];
}

static __device__ __forceinline__ Fr hash2(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr &a, const Fr &b) {
    Fr s[3] = {a, b, Fr::zero()};
    PoseidonPerm<3>::run(s, tab, f, p);
    return s[0];
}

// one Merkle level: out[i] = H(in[2 i], in[2 i + 1]), n_out parents
__global__ __launch_bounds__(POS_THREADS) void poseidon_level_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr *__restrict__ in, size_t n_out,
                                                                      Fr *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    out[i] = hash2(tab, f, p, in[2 * i], in[2 * i + 1]);
}

// poseidon.rs:121-132, one proof per lane: bit j of index picks [sibling, root] (set) or [root, sibling]
__global__ __launch_bounds__(POS_THREADS) void poseidon_proof_root_kernel(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr *__restrict__ leaves,
                                                                           const Fr *__restrict__ siblings, const uint64_t *__restrict__ indices, uint32_t depth,
                                                                           size_t n, Fr *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr root = leaves[i];
    const uint64_t idx = indices[i];
#pragma nounroll
    for (uint32_t j = 0; j < depth; j++) {
        const Fr sib = siblings[i * depth + j];
        const bool right = (idx >> j) & 1;
        Fr s[3];
#pragma unroll
        for (int k = 0; k < 8; k++) { s[0].v[k] = right ? sib.v[k] : root.v[k]; s[1].v[k] = right ? root.v[k] : sib.v[k]; s[2].v[k] = 0; }
        PoseidonPerm<3>::run(s, tab, f, p);
        root = s[0];
    }
    out[i] = root;
}

// the depth siblings of each requested leaf out of a built tree (levels one behind the other, leaves first): no hashing.
// An index >= 2^depth reads nothing, writes zeros and raises *bad.
__global__ __launch_bounds__(POS_THREADS) void merkle_siblings_kernel(const Fr *__restrict__ nodes, uint32_t depth, const uint64_t *__restrict__ indices, size_t n,
                                                                       Fr *__restrict__ out, uint32_t *bad) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * depth) return;
    const size_t pr = g / depth;
    const uint32_t j = (uint32_t)(g % depth);
    const uint64_t idx = indices[pr];
    if (idx >> depth) { if (j == 0) atomicOr(bad, 1u); out[g] = Fr::zero(); return; }
    const uint64_t off = ((uint64_t)2 << depth) - ((uint64_t)2 << (depth - j));     // the nodes of the levels below level j
    out[g] = nodes[off + ((idx >> j) ^ 1)];
}

// ------------------------------------------------------------------------------------------ host: Keccak-256, ChaCha20 (published specifications)
static inline uint64_t rol64(uint64_t v, unsigned n) { n &= 63; return n ? (v << n) | (v >> (64 - n)) : v; }

static void keccak_f1600(uint64_t a[25]) {       // a[x + 5 y]
    static uint64_t rc[24]; static unsigned rot[25]; static bool init = false;
    if (!init) {
        unsigned lfsr = 1;
        for (int r = 0; r < 24; r++) {
            uint64_t v = 0;
            for (int j = 0; j < 7; j++) {
                if (lfsr & 1) v ^= (uint64_t)1 << ((1u << j) - 1);
                lfsr = ((lfsr << 1) ^ ((lfsr & 0x80) ? 0x71 : 0)) & 0xff;
            }
            rc[r] = v;
        }
        for (int i = 0; i < 25; i++) rot[i] = 0;
        int x = 1, y = 0;
        for (int t = 0; t < 24; t++) { rot[x + 5 * y] = ((t + 1) * (t + 2) / 2) % 64; const int nx = y, ny = (2 * x + 3 * y) % 5; x = nx; y = ny; }
        init = true;
    }
    for (int r = 0; r < 24; r++) {
        uint64_t c[5], b[25];
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
        for (int x = 0; x < 5; x++) { const uint64_t d = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1); for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d; }
        for (int x = 0; x < 5; x++) for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol64(a[x + 5 * y], rot[x + 5 * y]);
        for (int x = 0; x < 5; x++) for (int y = 0; y < 5; y++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= rc[r];
    }
}

// Keccak-256 with the ORIGINAL padding 0x01 .. 0x80 (not SHA3-256's 0x06), rate 136
static void keccak256(const uint8_t *data, size_t len, uint8_t out[32]) {
    const size_t rate = 136;
    std::vector<uint8_t> msg(data, data + len);
    msg.push_back(0x01);
    while (msg.size() % rate) msg.push_back(0);
    msg.back() |= 0x80;
    uint64_t a[25] = {0};
    for (size_t off = 0; off < msg.size(); off += rate) {
        for (size_t i = 0; i < rate / 8; i++) { uint64_t w = 0; for (int b = 7; b >= 0; b--) w = (w << 8) | msg[off + 8 * i + b]; a[i] ^= w; }
        keccak_f1600(a);
    }
    for (int i = 0; i < 4; i++) for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(a[i] >> (8 * b));
}

static inline uint32_t rol32(uint32_t v, unsigned n) { return (v << n) | (v >> (32 - n)); }

// one ChaCha20 block: constants | 256-bit key | 64-bit block counter | 64-bit stream id
static void chacha20_block(const uint32_t key[8], uint64_t counter, uint64_t stream, uint32_t out[16]) {
    uint32_t s[16] = {0x61707865, 0x3320646e, 0x79622d32, 0x6b206574};
    for (int i = 0; i < 8; i++) s[4 + i] = key[i];
    s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = (uint32_t)stream; s[15] = (uint32_t)(stream >> 32);
    uint32_t w[16];
    for (int i = 0; i < 16; i++) w[i] = s[i];
    auto qr = [&](int a, int b, int c, int d) {
        w[a] += w[b]; w[d] = rol32(w[d] ^ w[a], 16);
        w[c] += w[d]; w[b] = rol32(w[b] ^ w[c], 12);
        w[a] += w[b]; w[d] = rol32(w[d] ^ w[a], 8);
        w[c] += w[d]; w[b] = rol32(w[b] ^ w[c], 7);
    };
    for (int r = 0; r < 10; r++) {
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
    }
    for (int i = 0; i < 16; i++) out[i] = w[i] + s[i];
}

// seedbox/src/lib.rs: ChaCha20 keyed with Keccak-256(salt); only next_u64 is drawn, so a value never straddles two blocks
struct Seedbox {
    uint32_t key[8]; uint64_t counter = 0; uint32_t buf[16]; int pos = 16;
    Seedbox(const uint8_t *salt, size_t len) {
        uint8_t h[32]; keccak256(salt, len, h);
        for (int i = 0; i < 8; i++) key[i] = (uint32_t)h[4 * i] | (uint32_t)h[4 * i + 1] << 8 | (uint32_t)h[4 * i + 2] << 16 | (uint32_t)h[4 * i + 3] << 24;
    }
    uint64_t next_u64() {
        if (pos >= 16) { chacha20_block(key, counter++, 0, buf); pos = 0; }
        const uint64_t v = (uint64_t)buf[pos] | (uint64_t)buf[pos + 1] << 32;
        pos += 2;
        return v;
    }
    // ff-uint/src/num/mod.rs:286-303: four limbs, the top two bits shaved, accepted below r; the sample IS the Montgomery image
    Fr gen_fr() {
        for (;;) {
            uint64_t l[4];
            for (int i = 0; i < 4; i++) l[i] = next_u64();
            l[3] &= ~(uint64_t)0 >> 2;
            Fr r;
            for (int i = 0; i < 4; i++) { r.v[2 * i] = (uint32_t)l[i]; r.v[2 * i + 1] = (uint32_t)(l[i] >> 32); }
            if (fr_below_modulus(r)) return r;
        }
    }
    static bool fr_below_modulus(const Fr &a) {
        for (int i = 7; i >= 0; i--) { const uint32_t q = FrParams::p(i); if (a.v[i] != q) return a.v[i] < q; }
        return false;
    }
};

static inline Fr fr_from_limbs(const uint64_t *l) {
    Fr r;
    for (int i = 0; i < 4; i++) { r.v[2 * i] = (uint32_t)l[i]; r.v[2 * i + 1] = (uint32_t)(l[i] >> 32); }
    return r;
}
static inline void fr_to_limbs(const Fr &a, uint64_t *l) { for (int i = 0; i < 4; i++) l[i] = (uint64_t)a.v[2 * i] | (uint64_t)a.v[2 * i + 1] << 32; }

static inline int dims_ok(uint32_t t, uint32_t f, uint32_t p) { return t >= 2 && t <= POS_MAX_T && (uint64_t)f + p != 0 && (uint64_t)f + p <= 4096; }

// ------------------------------------------------------------------------------------------ host drivers
// the parameters travel with every call: <= 20 KB at the head of ctx->misc, behind a 64-byte slot for the error flag of the sibling gather
struct PosDev { const Fr *tab; uint32_t *flag; };

static int pos_upload(fk_ctx *ctx, const fk_poseidon *h, PosDev *d) {
    const size_t bytes = h->tab.size() * sizeof(Fr);
    FK_HIP(ctx, ctx->misc.reserve(64 + bytes));
    FK_HIP(ctx, hipMemcpyAsync((uint8_t *)ctx->misc.p + 64, h->tab.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    d->tab = (const Fr *)((uint8_t *)ctx->misc.p + 64);
    d->flag = ctx->misc.as<uint32_t>();
    return FK_OK;
}

static inline unsigned pos_blocks(size_t n) { return (unsigned)((n + POS_THREADS - 1) / POS_THREADS); }

template <int T>
static void launch_hash(fk_ctx *ctx, const PosDev &d, const fk_poseidon *h, const Fr *in, uint32_t n_inputs, size_t n, Fr *out) {
    hipLaunchKernelGGL(poseidon_hash_kernel<T>, dim3(pos_blocks(n)), dim3(POS_THREADS), 0, ctx->stream, d.tab, h->f, h->p, in, n_inputs, n, out);
}
template <int T>
static void launch_sponge(fk_ctx *ctx, const PosDev &d, const fk_poseidon *h, const Fr *in, uint64_t len, size_t n, Fr *out) {
    hipLaunchKernelGGL(poseidon_sponge_kernel<T>, dim3(pos_blocks(n)), dim3(POS_THREADS), 0, ctx->stream, d.tab, h->f, h->p, in, len, Fr::from_u64(len), n, out);
}

// t = 2 .. 6 and 8 are instantiated
#define FK_POS_DISPATCH(t, CALL)                                                              \
    switch (t) {                                                                              \
    case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                   \
    case 5: CALL(5); break; case 6: CALL(6); break; case 8: CALL(8); break;                   \
    default: FK_SET_ERR(ctx, FK_ERR_UNSUPPORTED, "poseidon: no kernel is built for t = %u (built: 2, 3, 4, 5, 6, 8)", (unsigned)(t)); \
    }

static int hash_batch_dev(fk_ctx *ctx, const fk_poseidon *h, const Fr *d_in, uint32_t n_inputs, size_t n, Fr *d_out) {
    if (n > ((size_t)1 << 31) * POS_THREADS) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "poseidon: batch too large");
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
#define CALL(T) launch_hash<T>(ctx, d, h, d_in, n_inputs, n, d_out)
    FK_POS_DISPATCH(h->t, CALL)
#undef CALL
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "poseidon_hash_kernel");
    return FK_OK;
}

static int sponge_batch_dev(fk_ctx *ctx, const fk_poseidon *h, const Fr *d_in, uint64_t len, size_t n, Fr *d_out) {
    if (n > ((size_t)1 << 31) * POS_THREADS) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "poseidon: batch too large");
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
#define CALL(T) launch_sponge<T>(ctx, d, h, d_in, len, n, d_out)
    FK_POS_DISPATCH(h->t, CALL)
#undef CALL
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "poseidon_sponge_kernel");
    return FK_OK;
}

// d_nodes: 2^(L + 1) - 1 elements, L = ceil(log2 n_leaves); level 0 = the leaves (already in place), the padding is written here
static int merkle_tree_dev(fk_ctx *ctx, const fk_poseidon *h, Fr *d_nodes, uint64_t n_leaves, uint32_t L) {
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
    const uint64_t width = (uint64_t)1 << L;
    if (width > n_leaves) FK_HIP(ctx, hipMemsetAsync(d_nodes + n_leaves, 0, (width - n_leaves) * sizeof(Fr), ctx->stream));
    // One launch per level down to the root.  A single-workgroup kernel for the levels under 1024 nodes was measured and dropped: a level of few
    // hashes costs the latency of ONE hash (~0.45 ms) either way, ten launches add nothing that shows.
    Fr *in = d_nodes;
    for (uint64_t w = width; w > 1; w >>= 1) {
        hipLaunchKernelGGL(poseidon_level_kernel, dim3(pos_blocks(w >> 1)), dim3(POS_THREADS), 0, ctx->stream, d.tab, h->f, h->p, (const Fr *)in, (size_t)(w >> 1), in + w);
        in += w;
    }
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "poseidon_level_kernel");
    return FK_OK;
}

static int proof_roots_dev(fk_ctx *ctx, const fk_poseidon *h, const Fr *d_leaves, const Fr *d_sib, const uint64_t *d_idx, uint32_t depth, size_t n, Fr *d_out) {
    PosDev d; FK_TRY(pos_upload(ctx, h, &d));
    hipLaunchKernelGGL(poseidon_proof_root_kernel, dim3(pos_blocks(n)), dim3(POS_THREADS), 0, ctx->stream, d.tab, h->f, h->p, d_leaves, d_sib, d_idx, depth, n, d_out);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "poseidon_proof_root_kernel");
    return FK_OK;
}

static int tree_args(fk_ctx *ctx, const fk_poseidon *h, uint64_t n_leaves, uint32_t *L) {
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (h->t != 3) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: the tree hashes pairs with t = 3 parameters (got t = %u)", h->t);
    if (n_leaves == 0) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: a tree has at least one leaf");
    if (n_leaves > ((uint64_t)1 << POS_MAX_TREE_DEPTH)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: too many leaves");
    *L = ceil_log2_u64(n_leaves);
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

// ------------------------------------------------------------------------------------------ parameters (host only)
int fk_poseidon_params_new(uint32_t t, uint32_t f, uint32_t p, const char *salt, fk_poseidon **out) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    if (!out) return FK_ERR_BAD_ARG;
    *out = nullptr;
    if (!dims_ok(t, f, p)) { tls_error() = "poseidon: t must be 2..8 and f + p 1..4096"; return FK_ERR_BAD_ARG; }
    const std::string seed = "fawkes_poseidon(t=" + std::to_string(t) + ",f=" + std::to_string(f) + ",p=" + std::to_string(p) + ",salt=" + (salt ? salt : "") + ")";
    Seedbox sb((const uint8_t *)seed.data(), seed.size());
    fk_poseidon *h = new fk_poseidon();
    h->t = t; h->f = f; h->p = p;
    const size_t nc = (size_t)(f + p) * t;
    h->tab.resize(nc + (size_t)t * t);
    for (size_t i = 0; i < nc; i++) h->tab[i] = sb.gen_fr();
    Fr x[POS_MAX_T], y[POS_MAX_T];
    for (uint32_t i = 0; i < t; i++) x[i] = sb.gen_fr();
    for (uint32_t i = 0; i < t; i++) y[i] = sb.gen_fr();
    for (uint32_t i = 0; i < t; i++)
        for (uint32_t j = 0; j < t; j++) {
            const Fr s = Fr::add(x[i], y[j]);
            if (s.is_zero()) { delete h; tls_error() = "poseidon: x[i] + y[j] = 0, the matrix does not exist for this salt"; return FK_ERR_BAD_ARG; }
            h->tab[nc + (size_t)i * t + j] = Fr::inv(s);
        }
    *out = h;
    return FK_OK;
}); }

int fk_poseidon_params_load(uint32_t t, uint32_t f, uint32_t p, const uint64_t *c, const uint64_t *m, fk_poseidon **out) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    if (!out) return FK_ERR_BAD_ARG;
    *out = nullptr;
    if (!dims_ok(t, f, p) || !c || !m) { tls_error() = "poseidon: t must be 2..8, f + p 1..4096, c and m given"; return FK_ERR_BAD_ARG; }
    const size_t nc = (size_t)(f + p) * t, nm = (size_t)t * t;
    std::vector<Fr> tab(nc + nm);
    for (size_t i = 0; i < nc + nm; i++) {
        tab[i] = fr_from_limbs(i < nc ? c + 4 * i : m + 4 * (i - nc));
        if (!Seedbox::fr_below_modulus(tab[i])) { tls_error() = "poseidon: " + std::string(i < nc ? "constant " : "matrix entry ") + std::to_string(i < nc ? i : i - nc) + " is not below the modulus"; return FK_ERR_FORMAT; }
    }
    fk_poseidon *h = new fk_poseidon();
    h->t = t; h->f = f; h->p = p; h->tab.swap(tab);
    *out = h;
    return FK_OK;
}); }

int fk_poseidon_params_get(const fk_poseidon *h, uint32_t dims[3], uint64_t *c, uint64_t *m) {
    if (!h || !dims) return FK_ERR_BAD_ARG;
    dims[0] = h->t; dims[1] = h->f; dims[2] = h->p;
    const size_t nc = (size_t)(h->f + h->p) * h->t, nm = (size_t)h->t * h->t;
    if (c) for (size_t i = 0; i < nc; i++) fr_to_limbs(h->tab[i], c + 4 * i);
    if (m) for (size_t i = 0; i < nm; i++) fr_to_limbs(h->tab[nc + i], m + 4 * i);
    return FK_OK;
}

void fk_poseidon_free(fk_poseidon *h) { delete h; }

// ------------------------------------------------------------------------------------------ batch hashes
int fk_poseidon_hash_batch_dev(fk_ctx *ctx, const fk_poseidon *h, const void *d_inputs, uint32_t n_inputs, size_t n, void *d_out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (n_inputs == 0 || n_inputs >= h->t) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "poseidon: 0 < n_inputs < t required (n_inputs = %u, t = %u)", n_inputs, h->t);
    if (!n) return FK_OK;
    if (!d_inputs || !d_out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return hash_batch_dev(ctx, h, (const Fr *)d_inputs, n_inputs, n, (Fr *)d_out);
}); }

int fk_poseidon_hash_batch(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *inputs, uint32_t n_inputs, size_t n, uint64_t *out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (n_inputs == 0 || n_inputs >= h->t) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "poseidon: 0 < n_inputs < t required (n_inputs = %u, t = %u)", n_inputs, h->t);
    if (!n) return FK_OK;
    if (!inputs || !out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = n * n_inputs * sizeof(Fr), out_bytes = n * sizeof(Fr);
    FK_HIP(ctx, ctx->stage_a.reserve(in_bytes)); FK_HIP(ctx, ctx->stage_b.reserve(out_bytes));
    FK_HIP(ctx, hipMemcpyAsync(ctx->stage_a.p, inputs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    FK_TRY(hash_batch_dev(ctx, h, ctx->stage_a.as<Fr>(), n_inputs, n, ctx->stage_b.as<Fr>()));
    FK_HIP(ctx, hipMemcpyAsync(out, ctx->stage_b.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

int fk_poseidon_sponge_batch(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *inputs, uint64_t len, size_t n, uint64_t *out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (!n) return FK_OK;
    if (!out || (len && !inputs)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (len > ((uint64_t)1 << 40) / n) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "poseidon: sponge batch too large");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = n * len * sizeof(Fr), out_bytes = n * sizeof(Fr);
    FK_HIP(ctx, ctx->stage_a.reserve(in_bytes + sizeof(Fr))); FK_HIP(ctx, ctx->stage_b.reserve(out_bytes));
    if (in_bytes) FK_HIP(ctx, hipMemcpyAsync(ctx->stage_a.p, inputs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    FK_TRY(sponge_batch_dev(ctx, h, ctx->stage_a.as<Fr>(), len, n, ctx->stage_b.as<Fr>()));
    FK_HIP(ctx, hipMemcpyAsync(out, ctx->stage_b.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

// ------------------------------------------------------------------------------------------ Merkle trees
int fk_poseidon_merkle_tree_dev(fk_ctx *ctx, const fk_poseidon *h, const void *d_leaves, uint64_t n_leaves, void *d_nodes) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    uint32_t L = 0;
    FK_TRY(tree_args(ctx, h, n_leaves, &L));
    if (!d_leaves || !d_nodes) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    if (d_leaves != d_nodes) FK_HIP(ctx, hipMemcpyAsync(d_nodes, d_leaves, n_leaves * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    return merkle_tree_dev(ctx, h, (Fr *)d_nodes, n_leaves, L);
}); }

int fk_poseidon_merkle_root(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *leaves, uint64_t n_leaves, uint64_t *out_root) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    uint32_t L = 0;
    FK_TRY(tree_args(ctx, h, n_leaves, &L));
    if (!leaves || !out_root) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t total = ((uint64_t)2 << L) - 1;
    FK_HIP(ctx, ctx->stage_a.reserve(total * sizeof(Fr)));
    FK_HIP(ctx, hipMemcpyAsync(ctx->stage_a.p, leaves, n_leaves * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    FK_TRY(merkle_tree_dev(ctx, h, ctx->stage_a.as<Fr>(), n_leaves, L));
    FK_HIP(ctx, hipMemcpyAsync(out_root, ctx->stage_a.as<Fr>() + (total - 1), sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

int fk_poseidon_merkle_proofs_dev(fk_ctx *ctx, const void *d_nodes, uint32_t depth, const void *d_indices, size_t n, void *d_siblings) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (depth > POS_MAX_TREE_DEPTH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: depth %u is larger than any tree in device memory (max %u)", depth, POS_MAX_TREE_DEPTH);
    if (!n) return FK_OK;
    if (!d_nodes || !d_indices) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (n > ((size_t)1 << 36)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: too many proofs");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    FK_HIP(ctx, ctx->misc.reserve(64));
    uint32_t *flag = ctx->misc.as<uint32_t>();
    if (depth == 0) {       // no siblings to gather: only the indices are checked (all must be 0), on the host side of a small copy
        std::vector<uint64_t> idx(n);
        FK_HIP(ctx, hipMemcpyAsync(idx.data(), d_indices, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; i++) if (idx[i]) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: proof %zu has leaf index %llu, the tree has 1 leaf", i, (unsigned long long)idx[i]);
        return FK_OK;
    }
    if (!d_siblings) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(merkle_siblings_kernel, dim3(pos_blocks(n * depth)), dim3(POS_THREADS), 0, ctx->stream, (const Fr *)d_nodes, depth, (const uint64_t *)d_indices, n,
                       (Fr *)d_siblings, flag);
    FK_HIP(ctx, hipGetLastError());
    uint32_t bad = 0;
    FK_HIP(ctx, hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: a leaf index is not below 2^%u (its siblings were written as zeros, nothing was read)", depth);
    return FK_OK;
}); }

static int proof_args(fk_ctx *ctx, const fk_poseidon *h, uint32_t depth) {
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (h->t != 3) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: a proof hashes pairs with t = 3 parameters (got t = %u)", h->t);
    if (depth > 64) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: depth <= 64 required (a leaf index has 64 bits)");
    return FK_OK;
}

int fk_poseidon_merkle_proof_roots_dev(fk_ctx *ctx, const fk_poseidon *h, const void *d_leaves, const void *d_siblings, const void *d_indices, uint32_t depth, size_t n,
                                       void *d_out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(proof_args(ctx, h, depth));
    if (!n) return FK_OK;
    if (!d_leaves || !d_out || (depth && (!d_siblings || !d_indices))) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    if (depth == 0) { if (d_out != d_leaves) FK_HIP(ctx, hipMemcpyAsync(d_out, d_leaves, n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream)); return FK_OK; }
    return proof_roots_dev(ctx, h, (const Fr *)d_leaves, (const Fr *)d_siblings, (const uint64_t *)d_indices, depth, n, (Fr *)d_out);
}); }

int fk_poseidon_merkle_proof_roots(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *leaves, const uint64_t *siblings, const uint64_t *indices, uint32_t depth, size_t n,
                                   uint64_t *out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    FK_TRY(proof_args(ctx, h, depth));
    if (!n) return FK_OK;
    if (!leaves || !out || (depth && (!siblings || !indices))) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (depth == 0) { memmove(out, leaves, n * sizeof(Fr)); return FK_OK; }
    if (n > ((size_t)1 << 34)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: too many proofs");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lb = n * sizeof(Fr), sb = n * depth * sizeof(Fr), ib = n * sizeof(uint64_t);
    FK_HIP(ctx, ctx->stage_a.reserve(lb)); FK_HIP(ctx, ctx->stage_b.reserve(sb)); FK_HIP(ctx, ctx->stage_c.reserve(ib)); FK_HIP(ctx, ctx->stage_d.reserve(lb));
    FK_HIP(ctx, hipMemcpyAsync(ctx->stage_a.p, leaves, lb, hipMemcpyHostToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(ctx->stage_b.p, siblings, sb, hipMemcpyHostToDevice, ctx->stream));
    FK_HIP(ctx, hipMemcpyAsync(ctx->stage_c.p, indices, ib, hipMemcpyHostToDevice, ctx->stream));
    FK_TRY(proof_roots_dev(ctx, h, ctx->stage_a.as<Fr>(), ctx->stage_b.as<Fr>(), ctx->stage_c.as<uint64_t>(), depth, n, ctx->stage_d.as<Fr>()));
    FK_HIP(ctx, hipMemcpyAsync(out, ctx->stage_d.p, lb, hipMemcpyDeviceToHost, ctx->stream));
    FK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FK_OK;
}); }

}  // extern "C"
