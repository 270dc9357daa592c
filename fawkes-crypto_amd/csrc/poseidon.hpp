// Shared by poseidon.hip and eddsa.hip: the parameter object, the permutation (device), and the host helpers that derive library
// constants from the reference's seedbox (Keccak-256, ChaCha20) and move field elements across the C ABI.
#pragma once
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

static __device__ __forceinline__ Fr hash2(const Fr *__restrict__ tab, uint32_t f, uint32_t p, const Fr &a, const Fr &b) {
    Fr s[3] = {a, b, Fr::zero()};
    PoseidonPerm<3>::run(s, tab, f, p);
    return s[0];
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

static FK_HD uint32_t rol32(uint32_t v, unsigned n) { return (v << n) | (v >> (32 - n)); }

// one ChaCha20 block: constants | 256-bit key | 64-bit block counter | 64-bit stream id (host and device: ceremony.hip draws weights on both)
static FK_HD void chacha20_block(const uint32_t key[8], uint64_t counter, uint64_t stream, uint32_t out[16]) {
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
// The head of ctx->misc, as every hashing and signature call lays it out: a slot for the error flag (sibling gather, update's index check) |
// with a curve record: its slot (eddsa.hip) | the Poseidon table.  The parameters travel with every call: <= 20 KB.
static constexpr size_t MISC_FLAG_SLOT = 64, JJ_CONST_SLOT = 512;
struct PosDev { const Fr *tab; uint32_t *flag; const void *curve; };

// h, curve: what to upload (either may be null; without a curve record the table follows the flag slot at once)
static int misc_head(fk_ctx *ctx, const fk_poseidon *h, const void *curve, size_t curve_bytes, PosDev *d) {
    const size_t tab_off = MISC_FLAG_SLOT + (curve ? JJ_CONST_SLOT : 0), tab_bytes = h ? h->tab.size() * sizeof(Fr) : 0;
    FK_HIP(ctx, ctx->misc.reserve(tab_off + tab_bytes));
    uint8_t *base = ctx->misc.as<uint8_t>();
    if (curve) FK_HIP(ctx, hipMemcpyAsync(base + MISC_FLAG_SLOT, curve, curve_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (h) FK_HIP(ctx, hipMemcpyAsync(base + tab_off, h->tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    *d = PosDev{(const Fr *)(base + tab_off), (uint32_t *)base, base + MISC_FLAG_SLOT};
    return FK_OK;
}
static int pos_upload(fk_ctx *ctx, const fk_poseidon *h, PosDev *d) { return misc_head(ctx, h, nullptr, 0, d); }

static inline unsigned pos_blocks(size_t n) { return (unsigned)((n + POS_THREADS - 1) / POS_THREADS); }

}  // namespace fk
