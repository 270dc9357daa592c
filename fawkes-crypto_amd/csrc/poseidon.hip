// Poseidon over BN254 Fr on the device: batch hashes, the sponge, Merkle trees and Merkle proof roots -- the witness side of the
// rollup workload (native/poseidon.rs: PoseidonParams::new_with_salt, poseidon, poseidon_sponge, poseidon_merkle_proof_root,
// poseidon_merkle_tree_root).  One hash per lane with the state in registers; the round constants and the MDS matrix are the same
// for every lane and are read through wave-uniform indices of a const __restrict__ table (scalar loads).  Rounds are a run-time loop.
//
// Products per hash: (f t + p) * 3 for the S-boxes (x^5 = two squarings and a product) plus (f + p) * t^2 for the mix -- 780 at
// (t, f, p) = (3, 8, 53).  Mix rows: by default each row of the matrix product takes ONE Montgomery reduction per group of up to four
// columns (dot4 / mulsum of field.hpp: canonical operands, sum of k <= 4 products below k p^2, reduced below (1 + 0.19 k) p, one
// conditional subtraction); -DFK_POSEIDON_PLAIN_MIX builds the product-by-product form (same canonical values, hence same bytes).
#include "poseidon.hpp"

namespace fk {

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
    FK_TRY(scratch_claim(ctx, "poseidon hash"));
    const size_t in_bytes = n * n_inputs * sizeof(Fr), out_bytes = n * sizeof(Fr);
    HostStage st{ctx};
    const Fr *d_in; Fr *d_out;
    FK_TRY(st.in(ctx->stage_a, inputs, in_bytes, &d_in)); FK_TRY(st.room(ctx->stage_b, out_bytes, &d_out));
    FK_TRY(hash_batch_dev(ctx, h, d_in, n_inputs, n, d_out));
    return st.out(out, d_out, out_bytes);
}); }

int fk_poseidon_sponge_batch(fk_ctx *ctx, const fk_poseidon *h, const uint64_t *inputs, uint64_t len, size_t n, uint64_t *out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!h) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (!n) return FK_OK;
    if (!out || (len && !inputs)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (len > ((uint64_t)1 << 40) / n) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "poseidon: sponge batch too large");
    FK_TRY(scratch_claim(ctx, "poseidon sponge"));
    const size_t in_bytes = n * len * sizeof(Fr), out_bytes = n * sizeof(Fr);
    HostStage st{ctx};
    const Fr *d_in; Fr *d_out;
    FK_TRY(st.use(ctx->stage_a, {in_bytes}, sizeof(Fr))); FK_TRY(st.in(inputs, in_bytes, &d_in)); FK_TRY(st.room(ctx->stage_b, out_bytes, &d_out));
    FK_TRY(sponge_batch_dev(ctx, h, d_in, len, n, d_out));
    return st.out(out, d_out, out_bytes);
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
    FK_TRY(scratch_claim(ctx, "merkle root"));
    const uint64_t total = ((uint64_t)2 << L) - 1;
    HostStage st{ctx};
    Fr *d_nodes;
    FK_TRY(st.use(ctx->stage_a, {total * sizeof(Fr)})); FK_TRY(st.in(leaves, n_leaves * sizeof(Fr), &d_nodes));      // the leaves at the head of the node array
    FK_TRY(merkle_tree_dev(ctx, h, d_nodes, n_leaves, L));
    return st.out(out_root, d_nodes + (total - 1), sizeof(Fr));
}); }

int fk_poseidon_merkle_proofs_dev(fk_ctx *ctx, const void *d_nodes, uint32_t depth, const void *d_indices, size_t n, void *d_siblings) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (depth > POS_MAX_TREE_DEPTH) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: depth %u is larger than any tree in device memory (max %u)", depth, POS_MAX_TREE_DEPTH);
    if (!n) return FK_OK;
    if (!d_nodes || !d_indices) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (n > ((size_t)1 << 36)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "merkle: too many proofs");
    FK_HIP(ctx, hipSetDevice(ctx->device));       // misc only: runs beside an early front
    PosDev m; FK_TRY(misc_head(ctx, nullptr, nullptr, 0, &m));
    uint32_t *flag = m.flag;
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
    FK_TRY(scratch_claim(ctx, "merkle proof roots"));
    const size_t lb = n * sizeof(Fr), sb = n * depth * sizeof(Fr), ib = n * sizeof(uint64_t);
    HostStage st{ctx};
    const Fr *d_leaves, *d_sib; const uint64_t *d_idx; Fr *d_out;
    FK_TRY(st.in(ctx->stage_a, leaves, lb, &d_leaves)); FK_TRY(st.in(ctx->stage_b, siblings, sb, &d_sib)); FK_TRY(st.in(ctx->stage_c, indices, ib, &d_idx));
    FK_TRY(st.room(ctx->stage_d, lb, &d_out));
    FK_TRY(proof_roots_dev(ctx, h, d_leaves, d_sib, d_idx, depth, n, d_out));
    return st.out(out, d_out, lb);
}); }

}  // extern "C"
