// Device witness generation (include/fawkes_hip_witness.h): the witness program of one instance of a batch circuit, interpreted once per
// copy -- what the reference does by re-running the circuit closure on `WitnessCS` for every proof (prover.rs:69-76).
//
// One copy per lane, one wave per workgroup (copies are few: 1741 transactions are 28 waves), as in eddsa.hip.  Every lane of every wave
// runs the same operation on its own copy: the program (operations, combination headers, terms, coefficient dictionary, the exponent
// r - 2) is read through wave-uniform addresses behind `const __restrict__` pointers, so those are scalar loads and every branch on them
// is a uniform branch; nothing diverges except the exit of the lanes past `copies` in the last wave.  The zero cases of DIV0 and INV0 need
// no branch at all: 0^(r - 2) = 0, and a select pins that down.
//
// A lane reads and writes its copy's variables straight in the tiled output order (ONE, every copy's inputs, every copy's aux): 32-byte
// gathers and stores at a stride of num_aux * 32 bytes between lanes, no scratch copy of the witness.  The loader prepares each linear
// combination for that: the terms on ONE are folded into one constant (a dictionary slot, no product), the terms with coefficient ONE
// come first (additions only), the others follow and go four at a time through Fr::dot4 (one Montgomery reduction per four products).
// Field addition is exact, so the order of the terms does not change the value.  The public inputs are pseudo-operations behind the last
// variable: the same loop writes them.
//
// Products per copy: one per term with a coefficient other than ONE, one per MUL / DIV0, 379 per inversion (253 squarings +
// 126 products, the a^(r - 2) chain of eddsa.hip), one per run of BITs (from_mont).
#include "poseidon.hpp"
#include "../../include/fawkes_hip_witness.h"
#include <string>
#include <unordered_map>

struct fk_witness_prog {
    uint32_t num_input = 0, num_aux = 0, n_given = 0, n_lc = 0, n_ops = 0;
    uint64_t nnz = 0, n_table = 0, evals = 0, invs = 0;
    int device = 0;
    void *d_blob = nullptr;           // one allocation: table | ops | lcs | terms | exponent
    const fk::Fr *d_table = nullptr;
    const uint4 *d_ops = nullptr, *d_lcs = nullptr;
    const uint2 *d_terms = nullptr;
    const uint32_t *d_einv = nullptr;
};

namespace fk {

static constexpr uint32_t W_THREADS = 64;
static constexpr uint32_t WOP_PUBLIC = 5;           // loader-made: Input(1 + arg1) = <arg0, z>
static constexpr uint32_t WOP_REUSE = 0x100;        // a BIT of the combination the BIT before it evaluated: its canonical value is still held
static constexpr uint32_t W_NONE = 0xffffffffu;
static constexpr int W_FR_BITS = 254;

// device image.  WOp = uint4 {op | flags, arg0, arg1, -}; WLc = uint4 {first term, end of the unit-coefficient terms, end, dictionary slot
// of the constant or W_NONE}; term = uint2 {aux index, dictionary slot}.

static __device__ __forceinline__ Fr w_sel(bool c, const Fr &a, const Fr &b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}

// <l, z> on this lane's copy; zc: the copy's aux variables
static __device__ __forceinline__ Fr w_eval(const uint4 h, const uint2 *__restrict__ terms, const Fr *__restrict__ table, const Fr *zc) {
    Fr acc = Fr::zero();
    if (h.w != W_NONE) acc = table[h.w];
    uint32_t k = h.x;
#pragma nounroll
    for (; k + 4 <= h.y; k += 4) {
        const Fr x0 = zc[terms[k].x], x1 = zc[terms[k + 1].x], x2 = zc[terms[k + 2].x], x3 = zc[terms[k + 3].x];
        Fr s, t;
        Fr::add2(x0, x1, x2, x3, s, t);
        acc = Fr::add(acc, Fr::add(s, t));
    }
#pragma nounroll
    for (; k < h.y; k++) acc = Fr::add(acc, zc[terms[k].x]);
#pragma nounroll
    for (; k + 4 <= h.z; k += 4) {
        const uint2 t0 = terms[k], t1 = terms[k + 1], t2 = terms[k + 2], t3 = terms[k + 3];
        const Fr x0 = zc[t0.x], x1 = zc[t1.x], x2 = zc[t2.x], x3 = zc[t3.x];
        acc = Fr::add(acc, Fr::dot4(table[t0.y], x0, table[t1.y], x1, table[t2.y], x2, table[t3.y], x3));
    }
#pragma nounroll
    for (; k < h.z; k++) { const uint2 t = terms[k]; acc = Fr::add(acc, Fr::mul(table[t.y], zc[t.x])); }
    return acc;
}

// a^(r - 2): the chain of eddsa.hip (jj::pow_uniform), the exponent's bits are the same in every lane; 0 -> 0
static __device__ __forceinline__ Fr w_inv0(const Fr &a, const uint32_t *__restrict__ e) {
    Fr acc = a;
#pragma nounroll
    for (int i = W_FR_BITS - 2; i >= 0; i--) {
        acc = Fr::sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = Fr::mul(acc, a);
    }
    return w_sel(a.is_zero(), Fr::zero(), acc);
}

__global__ __launch_bounds__(W_THREADS) void witness_kernel(const uint4 *__restrict__ ops, uint32_t n_ops, const uint4 *__restrict__ lcs, const uint2 *__restrict__ terms,
                                                           const Fr *__restrict__ table, const uint32_t *__restrict__ e_inv, const Fr *__restrict__ given,
                                                           uint32_t num_input, uint32_t num_aux, uint32_t n_given, uint32_t copies, Fr *z) {
    const uint32_t c = blockIdx.x * W_THREADS + threadIdx.x;
    if (c >= copies) return;
    if (c == 0) z[0] = Fr::one();
    Fr *zin = z + 1 + (size_t)c * (num_input - 1);
    Fr *zc = z + 1 + (size_t)copies * (num_input - 1) + (size_t)c * num_aux;
    const Fr *g = given + (size_t)c * n_given;
    Fr canon = Fr::zero();
#pragma nounroll
    for (uint32_t v = 0; v < n_ops; v++) {
        const uint4 o = ops[v];
        const uint32_t op = o.x & 0xffu;
        Fr out;
        if (op == FK_WOP_GIVEN) {
            out = g[o.y];
        } else {
            Fr a = Fr::zero(), b = Fr::zero();
            if (!(o.x & WOP_REUSE)) {
                const int two = (op == FK_WOP_MUL || op == FK_WOP_DIV0) && o.y != o.z;
#pragma nounroll
                for (int k = 0; k <= two; k++) {            // a loop, not two copies of the code
                    const Fr r = w_eval(lcs[k ? o.z : o.y], terms, table, zc);
                    if (k == 0) a = r; else b = r;
                }
                if (!two) b = a;
            }
            if (op == FK_WOP_BIT) {
                if (!(o.x & WOP_REUSE)) canon = Fr::from_mont(a);
                uint32_t w = 0;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) w = (o.z >> 5) == j ? canon.v[j] : w;       // no run-time index into a register array
                out = w_sel((w >> (o.z & 31)) & 1, Fr::one(), Fr::zero());
            } else if (op == WOP_PUBLIC) {
                out = a;
            } else {
                if (op != FK_WOP_MUL) {                     // DIV0: a / b; INV0: 1 / a
                    b = w_inv0(b, e_inv);
                    if (op == FK_WOP_INV0) a = Fr::one();
                }
                out = Fr::mul(a, b);
            }
        }
        Fr *dst = op == WOP_PUBLIC ? zin + o.z : zc + v;
        *dst = out;
    }
}

// ------------------------------------------------------------------------------------------ host: the check
static inline uint32_t lc_count(uint32_t op) { return op == FK_WOP_GIVEN ? 0 : (op == FK_WOP_MUL || op == FK_WOP_DIV0) ? 2 : 1; }

#define W_FAIL(code, ...) do { char _b[256]; snprintf(_b, sizeof _b, __VA_ARGS__); why = _b; return (code); } while (0)

// max_col[l]: the largest column combination l names (0: ONE alone, or nothing)
static int witness_check(const fk_witness_desc *d, std::string &why, std::vector<uint32_t> *max_col_out = nullptr) {
    if (!d) W_FAIL(FK_ERR_BAD_ARG, "witness program: null descriptor");
    if (d->num_input == 0) W_FAIL(FK_ERR_BAD_ARG, "witness program: num_input is 0 (it counts ONE)");
    if ((d->num_aux && (!d->op || !d->arg0 || !d->arg1)) || (d->num_input > 1 && !d->input_lc) || (d->n_lc && !d->lc_ptr))
        W_FAIL(FK_ERR_BAD_ARG, "witness program: a missing array");
    const uint64_t nnz = d->n_lc ? d->lc_ptr[d->n_lc] : 0;
    if (d->n_lc && d->lc_ptr[0] != 0) W_FAIL(FK_ERR_BAD_ARG, "witness program: lc_ptr does not start at 0");
    for (uint32_t l = 0; l < d->n_lc; l++)
        if (d->lc_ptr[l + 1] < d->lc_ptr[l]) W_FAIL(FK_ERR_BAD_ARG, "witness program: lc_ptr decreases at combination %u", l);
    if (nnz >= 0xffffffffull) W_FAIL(FK_ERR_BAD_ARG, "witness program: %llu terms do not fit 32-bit term indices", (unsigned long long)nnz);
    if (nnz && !d->lc_col) W_FAIL(FK_ERR_BAD_ARG, "witness program: a missing array");
    std::vector<uint32_t> max_col(d->n_lc, 0);
    for (uint32_t l = 0; l < d->n_lc; l++)
        for (uint64_t k = d->lc_ptr[l]; k < d->lc_ptr[l + 1]; k++) {
            const uint32_t col = d->lc_col[k];
            if (col > d->num_aux) W_FAIL(FK_ERR_BAD_ARG, "witness program: combination %u names column %u, the instance has %u aux variables", l, col, d->num_aux);
            if (col > max_col[l]) max_col[l] = col;
            if (d->lc_val && !Seedbox::fr_below_modulus(fr_from_limbs(d->lc_val + 4 * k)))
                W_FAIL(FK_ERR_FORMAT, "witness program: combination %u, term %llu: the coefficient image is not below the modulus", l, (unsigned long long)(k - d->lc_ptr[l]));
        }
    for (uint32_t v = 0; v < d->num_aux; v++) {
        const uint32_t op = d->op[v];
        if (op > FK_WOP_BIT) W_FAIL(FK_ERR_BAD_ARG, "witness program: variable %u: unknown opcode %u", v, op);
        if (op == FK_WOP_GIVEN) {
            if (d->arg0[v] >= d->n_given) W_FAIL(FK_ERR_BAD_ARG, "witness program: variable %u: given index %u, a row holds %u", v, d->arg0[v], d->n_given);
            continue;
        }
        for (uint32_t k = 0; k < lc_count(op); k++) {
            const uint32_t l = k ? d->arg1[v] : d->arg0[v];
            if (l >= d->n_lc) W_FAIL(FK_ERR_BAD_ARG, "witness program: variable %u: combination %u of %u", v, l, d->n_lc);
            if (max_col[l] > v) W_FAIL(FK_ERR_BAD_ARG, "witness program: variable %u: combination %u names Aux(%u), which is not an earlier variable", v, l, max_col[l] - 1);
        }
        if (op == FK_WOP_BIT && d->arg1[v] >= 256) W_FAIL(FK_ERR_BAD_ARG, "witness program: variable %u: bit index %u", v, d->arg1[v]);
    }
    for (uint32_t i = 0; i + 1 < d->num_input; i++)
        if (d->input_lc[i] >= d->n_lc) W_FAIL(FK_ERR_BAD_ARG, "witness program: input %u: combination %u of %u", i + 1, d->input_lc[i], d->n_lc);
    if (max_col_out) max_col_out->swap(max_col);
    return FK_OK;
}

// ------------------------------------------------------------------------------------------ host: the device image
struct WImage {
    std::vector<Fr> table;
    std::vector<uint4> ops, lcs;
    std::vector<uint2> terms;
    uint64_t evals = 0, invs = 0;
};

static int witness_image(const fk_witness_desc *d, WImage &im, std::string &why) {
    std::unordered_map<std::string, uint32_t> dict;
    const Fr one = Fr::one();
    auto slot = [&](const Fr &c) -> uint32_t {
        const std::string key((const char *)&c, 32);
        auto it = dict.find(key);
        if (it == dict.end()) { it = dict.emplace(key, (uint32_t)im.table.size()).first; im.table.push_back(c); }
        return it->second;
    };
    slot(one);                                                  // slot 0 = ONE
    const uint64_t nnz = d->n_lc ? d->lc_ptr[d->n_lc] : 0;
    im.terms.reserve(nnz); im.lcs.reserve(d->n_lc);
    std::vector<uint2> rest;
    for (uint32_t l = 0; l < d->n_lc; l++) {
        Fr konst = Fr::zero(); bool has_konst = false;
        const uint32_t lo = (uint32_t)im.terms.size();
        rest.clear();
        for (uint64_t k = d->lc_ptr[l]; k < d->lc_ptr[l + 1]; k++) {
            const Fr c = d->lc_val ? fr_from_limbs(d->lc_val + 4 * k) : one;
            const uint32_t col = d->lc_col[k];
            if (col == 0) { konst = Fr::add(konst, c); has_konst = true; continue; }
            const uint32_t s = slot(c);
            if (s == 0) im.terms.push_back(make_uint2(col - 1, 0)); else rest.push_back(make_uint2(col - 1, s));
        }
        const uint32_t unit_end = (uint32_t)im.terms.size();
        im.terms.insert(im.terms.end(), rest.begin(), rest.end());
        im.lcs.push_back(make_uint4(lo, unit_end, (uint32_t)im.terms.size(), has_konst ? slot(konst) : W_NONE));
    }
    if (im.table.size() >= 0xffffffffull) W_FAIL(FK_ERR_BAD_ARG, "witness program: too many distinct coefficients");
    im.ops.reserve((size_t)d->num_aux + d->num_input - 1);
    for (uint32_t v = 0; v < d->num_aux; v++) {
        const uint32_t op = d->op[v];
        uint32_t word = op;
        if (op == FK_WOP_BIT && v && d->op[v - 1] == FK_WOP_BIT && d->arg0[v - 1] == d->arg0[v]) word |= WOP_REUSE;
        else if (op != FK_WOP_GIVEN) im.evals += (lc_count(op) == 2 && d->arg0[v] != d->arg1[v]) ? 2 : 1;
        if (op == FK_WOP_DIV0 || op == FK_WOP_INV0) im.invs++;
        im.ops.push_back(make_uint4(word, d->arg0[v], d->arg1[v], 0));
    }
    for (uint32_t i = 0; i + 1 < d->num_input; i++) { im.ops.push_back(make_uint4(WOP_PUBLIC, d->input_lc[i], i, 0)); im.evals++; }
    return FK_OK;
}

static int witness_load(fk_ctx *ctx, const fk_witness_desc *d, fk_witness_prog **out) {
    std::string why;
    const int rc = witness_check(d, why);
    if (rc != FK_OK) { ctx->err = why; return rc; }
    WImage im;
    const int rc2 = witness_image(d, im, why);
    if (rc2 != FK_OK) { ctx->err = why; return rc2; }
    uint32_t e_inv[8]; uint32_t br = 2;
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)FrParams::p(i) - br; e_inv[i] = (uint32_t)t; br = (uint32_t)(t >> 63); }
    // every section starts 16-byte aligned (a section of 16-byte elements, or the last one)
    const size_t b_table = im.table.size() * sizeof(Fr), b_ops = im.ops.size() * sizeof(uint4), b_lcs = im.lcs.size() * sizeof(uint4),
                 b_terms = (im.terms.size() * sizeof(uint2) + 15) & ~(size_t)15, b_e = sizeof e_inv;
    std::vector<uint8_t> blob(b_table + b_ops + b_lcs + b_terms + b_e, 0);
    uint8_t *p = blob.data();
    memcpy(p, im.table.data(), b_table); p += b_table;
    if (b_ops) memcpy(p, im.ops.data(), b_ops);
    p += b_ops;
    if (b_lcs) memcpy(p, im.lcs.data(), b_lcs);
    p += b_lcs;
    if (!im.terms.empty()) memcpy(p, im.terms.data(), im.terms.size() * sizeof(uint2));
    p += b_terms;
    memcpy(p, e_inv, b_e);
    FK_HIP(ctx, hipSetDevice(ctx->device));
    fk_witness_prog *w = new fk_witness_prog;
    hipError_t e = hipMalloc(&w->d_blob, blob.size());
    if (e == hipSuccess) e = hipMemcpy(w->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (w->d_blob) (void)hipFree(w->d_blob);
        delete w;
        (void)hipGetLastError();
        FK_SET_ERR(ctx, e == hipErrorOutOfMemory ? FK_ERR_OOM : FK_ERR_HIP, "witness program: upload failed: %s", hipGetErrorString(e));
    }
    const uint8_t *q = (const uint8_t *)w->d_blob;
    w->d_table = (const Fr *)q; q += b_table;
    w->d_ops = (const uint4 *)q; q += b_ops;
    w->d_lcs = (const uint4 *)q; q += b_lcs;
    w->d_terms = (const uint2 *)q; q += b_terms;
    w->d_einv = (const uint32_t *)q;
    w->num_input = d->num_input; w->num_aux = d->num_aux; w->n_given = d->n_given; w->n_lc = d->n_lc; w->n_ops = (uint32_t)im.ops.size();
    w->nnz = d->n_lc ? d->lc_ptr[d->n_lc] : 0; w->n_table = im.table.size(); w->evals = im.evals; w->invs = im.invs;
    w->device = ctx->device;
    *out = w;
    return FK_OK;
}

// elements of the tiled witness, or 0 when the batch does not fit 32-bit variable indices (fk_r1cs_load_tiled's rule)
static uint64_t witness_len(const fk_witness_prog *w, uint32_t copies) {
    const uint64_t n = 1 + (uint64_t)copies * (w->num_input - 1) + (uint64_t)copies * w->num_aux;
    return n > 0xffffffffull ? 0 : n;
}

static int witness_run(fk_ctx *ctx, const fk_witness_prog *w, const void *d_given, uint32_t copies, void *d_z) {
    if (w->device != ctx->device) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "witness: the program is resident on device %d, the context runs device %d", w->device, ctx->device);
    if (!witness_len(w, copies))
        FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "witness: %u copies of this program do not fit 32-bit variable indices", copies);
    hipLaunchKernelGGL(witness_kernel, dim3((copies + W_THREADS - 1) / W_THREADS), dim3(W_THREADS), 0, ctx->stream, w->d_ops, w->n_ops, w->d_lcs, w->d_terms, w->d_table,
                       w->d_einv, (const Fr *)d_given, w->num_input, w->num_aux, w->n_given, copies, (Fr *)d_z);
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "witness_kernel");
    return FK_OK;
}

}  // namespace fk

using namespace fk;

extern "C" {

int fk_witness_program_check(const fk_witness_desc *desc) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    std::string why;
    const int rc = witness_check(desc, why);
    if (rc != FK_OK) tls_error() = why;
    return rc;
}); }

int fk_witness_program_load(fk_ctx *ctx, const fk_witness_desc *desc, fk_witness_prog **out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    return witness_load(ctx, desc, out);
}); }

int fk_witness_program_info(const fk_witness_prog *prog, uint64_t out[8]) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    if (!prog || !out) return FK_ERR_BAD_ARG;
    out[0] = prog->num_input; out[1] = prog->num_aux; out[2] = prog->n_given; out[3] = prog->n_lc;
    out[4] = prog->nnz; out[5] = prog->n_table; out[6] = prog->evals; out[7] = prog->invs;
    return FK_OK;
}); }

void fk_witness_program_free(fk_ctx *ctx, fk_witness_prog *prog) {
    if (!prog) return;
    (void)fk_guard(ctx, [&]() -> int {
        if (ctx) (void)hipSetDevice(ctx->device);
        if (prog->d_blob) (void)hipFree(prog->d_blob);
        delete prog;
        return FK_OK;
    });
}

int fk_witness_generate_dev(fk_ctx *ctx, const fk_witness_prog *prog, const void *d_given, uint32_t copies, void *d_z) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!prog) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (!copies) return FK_OK;
    if (!d_z || (prog->n_given && !d_given)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    return witness_run(ctx, prog, d_given, copies, d_z);
}); }

int fk_witness_generate(fk_ctx *ctx, const fk_witness_prog *prog, const uint64_t *given, uint32_t copies, uint64_t *z) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!prog) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    if (!copies) return FK_OK;
    if (!z || (prog->n_given && !given)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "null argument");
    const uint64_t len = witness_len(prog, copies);
    if (!len) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "witness: %u copies of this program do not fit 32-bit variable indices", copies);
    FK_TRY(scratch_claim(ctx, "witness"));
    const size_t gb = (size_t)copies * prog->n_given * sizeof(Fr), zb = (size_t)len * sizeof(Fr);
    HostStage st{ctx};
    const void *d_given; void *d_z;
    FK_TRY(st.use(ctx->stage_a, {gb}, gb ? 0 : sizeof(Fr))); FK_TRY(st.in(given, gb, &d_given)); FK_TRY(st.room(ctx->stage_b, zb, &d_z));
    FK_TRY(witness_run(ctx, prog, d_given, copies, d_z));
    return st.out(z, d_z, zb);
}); }

}  // extern "C"
