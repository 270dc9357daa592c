// Device-resident R1CS and the sparse evaluation  a = A z, b = B z, c = C z  (SURVEY.md section 8f, row 1).
//
// Replaces, for the prover, what bellman's ProvingAssignment does gate by gate on the CPU while
// fawkes streams the constraint system out of its brotli blob
// (/root/reference/fawkes-crypto/src/backend/bellman_groth16/mod.rs:92-99,
//  /root/reference/fawkes-crypto/src/circuit/r1cs/cs.rs:184-223; evaluation semantics SURVEY App. A.1):
// a_i = <A_i, z>, b_i = <B_i, z>, c_i = <C_i, z>, plus one `input_i * 0 = 0` row per input, and the
// three density maps, which are structural (a variable is marked when it is *visited*) and are therefore
// computed once at load time.
//
// Layout in HBM: CSR per matrix -- row_ptr u64[num_gates+1], col u32[nnz] (Input(i) -> i,
// Aux(j) -> num_input + j) and a coefficient DICTIONARY: fawkes LCs carry few distinct constants
// (1, -1, small integers, Poseidon MDS entries), so each term stores a u32 index into a table of unique
// 32-byte Montgomery values instead of the value itself: 8 B per term instead of 36 B, and the table
// stays in L2.  Index 0 is reserved for ONE (multiply skipped, exactly as bellman's eval does).
// Kernel: one lane per (matrix, row); HBM-bound gather of z (32 B per term).
#include "common.hpp"
#include <chrono>
#include <memory>

#include "spmv_plan.hpp"
#include "../../include/fawkes_hip_inspect.h"

namespace fk {

struct SpmvArgs {
    const uint64_t *ptr[3];
    const uint32_t *col[3];
    const uint32_t *cidx[3];
    Fr *out[3];
};

// G = 2^lg lanes share one row: lane s takes terms s, s + G, ... and the partial sums are folded with wave64 shuffles.
// Real circuits have long linear combinations (the eddsa verifier: 133 terms per gate on average, rows of up to 512), and
// with one lane per row a wave runs as long as its longest row; the synthetic rollup shape (1-2 terms per row) keeps G = 1.
//
// TILED: the CSR describes one instance of a batch circuit and row t is row t % base_gates of copy t / base_gates; the
// copy's variables are found by arithmetic (ONE shared, then every copy's inputs, then every copy's aux variables: the
// layout of a circuit that allocates the same gadget `copies` times), so a 4096-signature batch costs the memory of one.
struct TileDims { uint32_t base_gates, base_input, base_aux; };
// binned: bit k set = matrix k's gate rows belong to spmv_binned_kernel; this kernel then only writes the rows behind them
// SLICED: lane group tl evaluates row t = rank + W * tl and writes out[tl] (the cyclic slice of rank `rank` of W = 2^log_w)
template <bool TILED, bool SLICED>
__global__ __launch_bounds__(256) void spmv_kernel(SpmvArgs a, const Fr *table, const Fr *z, uint64_t num_gates, uint32_t num_input, uint32_t lg0, uint32_t lg1,
                                                   uint32_t lg2, TileDims td, uint32_t binned, uint32_t log_w, uint32_t rank) {
    const uint32_t mtx = blockIdx.y;
    const uint32_t lg = mtx == 0 ? lg0 : (mtx == 1 ? lg1 : lg2);
    const uint64_t tl = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> lg;
    const uint64_t t = SLICED ? rank + (tl << log_w) : tl;
    const uint32_t sub = threadIdx.x & ((1u << lg) - 1);
    const uint64_t rows = num_gates + num_input;
    if (t >= rows) return;                   // the lanes of a row group leave together (256 is a multiple of G)
    if (((binned >> mtx) & 1) && t < num_gates) return;
    const uint64_t *ptr = a.ptr[mtx]; const uint32_t *col = a.col[mtx]; const uint32_t *cidx = a.cidx[mtx];
    Fr acc = Fr::zero();
    if (t < num_gates) {
        uint32_t copy = 0; uint64_t row = t;
        if (TILED) { copy = (uint32_t)t / td.base_gates; row = (uint32_t)t - copy * td.base_gates; }
        const uint32_t in_off = copy * (td.base_input - 1), aux_off = num_input + copy * td.base_aux - td.base_input;
        for (uint64_t k = ptr[row] + sub, e = ptr[row + 1]; k < e; k += (uint64_t)1 << lg) {
            uint32_t cv = col[k];
            if (TILED && cv) cv += cv < td.base_input ? in_off : aux_off;
            Fr v = z[cv];
            const uint32_t ci = cidx[k];
            if (ci) v = Fr::mul(v, table[ci]);
            acc = Fr::add(acc, v);
        }
    } else if (mtx == 0 && sub == 0) {
        acc = z[t - num_gates];        // bellman's extra rows: input_i * 0 = 0
    }
    for (uint32_t off = (1u << lg) >> 1; off; off >>= 1) {
        Fr o;
#pragma unroll
        for (int i = 0; i < 8; i++) o.v[i] = (uint32_t)__shfl_down((int)acc.v[i], off, 64);
        acc = Fr::add(acc, o);
    }
    if (sub == 0) a.out[mtx][tl] = acc;
}

// Circuits built from Poseidon are bimodal: three quarters of the eddsa verifier's rows hold ONE term, the rest 128-512 (the
// MDS mixing is kept as lazily expanded linear combinations).  A wave runs as long as its longest row, so one lane-group
// size for a whole matrix wastes most lanes either way.  Here the rows of a matrix are split by length into classes with
// their own group size (1, 2, 4, 8 or 16 lanes per row: a lane gets 4 .. 7 terms) and sorted by length inside a class, so that the rows sharing a wave
// have (nearly) the same length; long rows take two terms per step through the dual-chain multiplier.  Segment s of the
// launch is one (matrix, class); a tiled system walks its copies in the outer order, so a copy's z stays in cache.
// SLICED (b.rowlist = the residue-grouped lists, b.first_block = this rank's plan): group index -> (copy, position in the
// residue group that copy needs); the row's result goes to out[(copy * base_gates + row) >> log_w].
#ifndef FK_SPMV_MINB
#define FK_SPMV_MINB 1      // workgroups per compute unit the register allocation is held to (256 lanes = one wave per SIMD each): see the kernel's comment
#endif
template <bool TILED, bool SLICED>
__global__ __launch_bounds__(256, FK_SPMV_MINB) void spmv_binned_kernel(SpmvArgs a, BinArgs b, const Fr *table, const Fr *z, uint32_t num_input, TileDims td, uint32_t copies, SliceArgs sl) {
    uint32_t s = 0;
    while (s + 1 < b.nseg && blockIdx.x >= b.first_block[s + 1]) s++;
    const uint32_t lg = b.lg[s], mtx = b.mtx[s], nr = b.n_rows[s];
    const uint64_t gidx = (uint64_t)(blockIdx.x - b.first_block[s]) * (256u >> lg) + (threadIdx.x >> lg);
    const uint32_t sub = threadIdx.x & ((1u << lg) - 1);
    uint32_t copy = 0, li = (uint32_t)gidx;
    if (SLICED) {
        const uint32_t T = sl.T[s];
        const uint64_t q = gidx / T;
        uint32_t rem = (uint32_t)(gidx - q * T), pp = 0;
        while (pp + 1 < sl.P && rem >= sl.cnt[s][sl.rho[pp]]) { rem -= sl.cnt[s][sl.rho[pp]]; pp++; }
        const uint64_t cp = q * sl.P + pp;
        if (cp >= copies || rem >= sl.cnt[s][sl.rho[pp]]) return;
        copy = (uint32_t)cp;
        li = sl.offs[s][sl.rho[pp]] + rem;
    } else {
        if (gidx >= (uint64_t)nr * copies) return;
        if (TILED) { copy = (uint32_t)(gidx / nr); li = (uint32_t)(gidx - (uint64_t)copy * nr); }
    }
    const uint32_t row = b.rowlist[mtx][b.list_off[s] + li];
    const uint32_t in_off = copy * (td.base_input - 1), aux_off = num_input + copy * td.base_aux - td.base_input;
    const uint64_t *ptr = a.ptr[mtx]; const uint32_t *col = a.col[mtx]; const uint32_t *cidx = a.cidx[mtx];
    const uint64_t e = ptr[row + 1];
    uint64_t k = ptr[row] + sub;
    const uint32_t G = 1u << lg;
    auto var = [&](uint32_t cv) -> uint32_t { if (TILED && cv) cv += cv < td.base_input ? in_off : aux_off; return cv; };
    Fr acc = Fr::zero();
    // four terms per step with ONE Montgomery reduction (Fp::dot4: 328 multiply-accumulates instead of 544) ...
    for (; k + 3 * (uint64_t)G < e; k += 4 * G) {
        const uint32_t c0 = var(col[k]), c1 = var(col[k + G]), c2 = var(col[k + 2 * G]), c3 = var(col[k + 3 * G]);
        const uint32_t i0 = cidx[k], i1 = cidx[k + G], i2 = cidx[k + 2 * G], i3 = cidx[k + 3 * G];
        acc = Fr::add(acc, Fr::dot4(z[c0], table[i0], z[c1], table[i1], z[c2], table[i2], z[c3], table[i3]));
    }           // (loading the NEXT step's indices ahead of this step's products was measured: 169.8 against 168.8 ms per proof)
    if (lg) {   // ... then two (one lane per row: the last terms one by one, ONE coefficients skipped)
        Fr acc1 = Fr::zero();
        for (; k + G < e; k += 2 * G) {        // table[0] is ONE: multiplying by it returns the (reduced) value itself
            const uint32_t c0 = var(col[k]), c1 = var(col[k + G]), i0 = cidx[k], i1 = cidx[k + G];
            Fr p0, p1;
            Fr::mul2(z[c0], table[i0], z[c1], table[i1], p0, p1);
            Fr::add2(acc, p0, acc1, p1, acc, acc1);
        }
        acc = Fr::add(acc, acc1);
    }
    for (; k < e; k += G) {
        const uint32_t cv = var(col[k]);
        Fr v = z[cv];
        const uint32_t ci = cidx[k];
        if (ci) v = Fr::mul(v, table[ci]);
        acc = Fr::add(acc, v);
    }
    for (uint32_t off = G >> 1; off; off >>= 1) {
        Fr o;
#pragma unroll
        for (int i = 0; i < 8; i++) o.v[i] = (uint32_t)__shfl_down((int)acc.v[i], off, 64);
        acc = Fr::add(acc, o);
    }
    if (sub == 0) a.out[mtx][((uint64_t)copy * td.base_gates + row) >> (SLICED ? sl.log_w : 0)] = acc;
}

// Batch circuits (TILED), rows of middling length the other way round: one WAVE per (instance row, block of 64 copies) -- lane l
// evaluates the row for copy 64 * cb + l.  Every lane of a wave then walks the SAME row: the trip count, the column and
// coefficient indices and the coefficients are wave-uniform (scalar loads, one copy in SGPRs), no lane is padding (a 33-term
// row shared by 16 lanes keeps them busy 33 / 48 of the time), there are no partial sums to fold, and four terms at a time
// share one Montgomery reduction.  What differs per lane is the copy's offset into z.  Measured on the benchmark's system
// (tools/spmv_rollup_probe.py, profiles/r03_spmv_rollup_probe.log): rows of 4 .. 31 terms 2.16 -> 1.78 ms, 32 .. 63 terms
// 4.58 -> 2.83 ms; rows of 64 terms and more are faster in the lane-group form (their 16 lanes read neighbouring variables of
// ONE copy; here 64 lanes read 64 copies' -- 3.72 -> 4.80 ms), single-term rows too, so those stay with spmv_binned_kernel.
// wavelist: the rows (matrix in the top two bits) in circuit order, so that what runs at one time reads a window of the
// same 64 copies' variables; copy block outermost.
__global__ __launch_bounds__(256) void spmv_tiled_wave_kernel(SpmvArgs a, const Fr *table, const Fr *z, uint32_t num_input, TileDims td, uint32_t copies,
                                                              const uint32_t *wavelist, uint32_t n_list, uint32_t n_waves) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (wave >= n_waves) return;
    const uint32_t cb = wave / n_list, ent = wavelist[wave - cb * n_list], mtx = ent >> 30, row = ent & 0x3fffffffu;
    const uint32_t c_raw = cb * 64 + lane;
    const bool active = c_raw < copies;
    const uint32_t copy = active ? c_raw : copies - 1;
    const uint32_t in_off = copy * (td.base_input - 1), aux_off = num_input + copy * td.base_aux - td.base_input;
    const uint64_t *ptr = a.ptr[mtx]; const uint32_t *col = a.col[mtx]; const uint32_t *cidx = a.cidx[mtx];
    auto var = [&](uint32_t cv) -> uint32_t { if (cv) cv += cv < td.base_input ? in_off : aux_off; return cv; };
    uint64_t k = ptr[row];
    const uint64_t e = ptr[row + 1];
    Fr acc = Fr::zero();
    for (; k + 3 < e; k += 4)
        acc = Fr::add(acc, Fr::dot4(z[var(col[k])], table[cidx[k]], z[var(col[k + 1])], table[cidx[k + 1]], z[var(col[k + 2])], table[cidx[k + 2]],
                                    z[var(col[k + 3])], table[cidx[k + 3]]));
    if (k + 1 < e) {
        Fr p0, p1;
        Fr::mul2(z[var(col[k])], table[cidx[k]], z[var(col[k + 1])], table[cidx[k + 1]], p0, p1);
        acc = Fr::add(acc, Fr::add(p0, p1));
        k += 2;
    }
    if (k < e) {
        Fr v = z[var(col[k])];
        const uint32_t ci = cidx[k];
        if (ci) v = Fr::mul(v, table[ci]);       // index 0 is ONE: bellman's eval skips that product, and so does every lane here
        acc = Fr::add(acc, v);
    }
    if (active) a.out[mtx][(uint64_t)copy * td.base_gates + row] = acc;
}

// the largest variable index each row window reads: terms [tb[j], tb[j + 1]) of a matrix belong to window j
struct WinBounds { uint64_t tb[fk_r1cs_dev::WIN_MAX + 1]; uint32_t k; };
__global__ __launch_bounds__(256) void col_window_max_kernel(const uint32_t *col, WinBounds wb, uint32_t *out) {
    const uint64_t n = wb.tb[wb.k];
    uint32_t w = 0, mx = 0; bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        while (i >= wb.tb[w + 1]) { if (any) atomicMax(&out[w], mx); mx = 0; any = false; w++; }
        const uint32_t c = col[i];
        if (c > mx) mx = c;
        any = true;
    }
    if (any) atomicMax(&out[w], mx);
}

// Repeated linear combinations (r1cs.hpp: the alias plan): one lane per alias copies the value spmv_binned_kernel (or spmv_kernel, for a
// source in a matrix that is not binned) wrote for the source row a moment ago on the same stream -- 8 + 32 + 32 bytes instead of a z
// gather, a table load and a multiply-accumulate per term.  A source is never an alias itself, so the lanes do not depend on each other.
__global__ __launch_bounds__(256) void spmv_alias_kernel(Fr *out0, Fr *out1, Fr *out2, const uint64_t *alias, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = alias[i];
    const uint32_t drow = (uint32_t)e, srow = drow - ((uint32_t)(e >> 32) & 0xffffu), dm = (uint32_t)(e >> 48) & 3u, sm = (uint32_t)(e >> 50) & 3u;
    const Fr *src = sm == 0 ? out0 : (sm == 1 ? out1 : out2);
    Fr *dst = dm == 0 ? out0 : (dm == 1 ? out1 : out2);
    dst[drow] = src[srow];
}

// one host array into an exactly-sized device array of its own (pad: elements allocated behind the n copied)
template <class T>
static int dev_upload(fk_ctx *ctx, DevArr<T> &d, const T *h, size_t n, size_t pad = 0) {
    if (d.alloc(n + pad) != hipSuccess) FK_SET_ERR(ctx, FK_ERR_OOM, "r1cs: device allocation failed");
    if (n && hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) FK_SET_ERR(ctx, FK_ERR_HIP, "r1cs: upload failed");
    return FK_OK;
}

// win_need of the row windows the plan cut (r1cs.hpp), from the uploaded columns: a host pass over 10^9 columns is what the kernel avoids
static int window_need(fk_ctx *ctx, const SpmvPlan &p, fk_r1cs_dev &r) {
    const uint32_t K = r.win_k;
    if (!K) return FK_OK;
    DevArr<uint32_t> d_mx;
    if (d_mx.alloc(K) != hipSuccess || hipMemset(d_mx, 0, K * 4) != hipSuccess) FK_SET_ERR(ctx, FK_ERR_OOM, "r1cs: device allocation failed");
    for (int k = 0; k < 3; k++) {
        WinBounds wb{}; wb.k = K;
        for (uint32_t j = 0; j <= K; j++) wb.tb[j] = p.ptr[k][r.win_row[j]];
        if (wb.tb[K]) hipLaunchKernelGGL(col_window_max_kernel, dim3(2048), dim3(256), 0, ctx->stream, r.col[k].p, wb, d_mx.p);
    }
    uint32_t mx[fk_r1cs_dev::WIN_MAX] = {0};
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(mx, d_mx, K * 4, hipMemcpyDeviceToHost) != hipSuccess)
        FK_SET_ERR(ctx, FK_ERR_HIP, "r1cs: window planning failed");
    uint64_t run = p.num_input;                          // the rows behind the gates (input_i * 0 = 0) read the inputs: part of the first piece
    for (uint32_t j = 0; j < K; j++) { run = std::max<uint64_t>(run, (uint64_t)mx[j] + 1); r.win_need[j] = j + 1 == K ? (uint64_t)p.num_input + p.num_aux : run; }
    return FK_OK;
}

// The loader: the plan's stages (spmv_plan.hpp) in their order, each followed by the upload of what it left; win_need and the A query's
// fingerprint come from the device.  The resident object owns every device array, so whatever ends the load early frees what was built.
static int r1cs_load_impl(fk_ctx *ctx, const fk_r1cs *cs, uint32_t copies, fk_r1cs_dev **out, const uint32_t *const *pre_cidx = nullptr,
                          const Fr *pre_table = nullptr, uint64_t n_pre_table = 0, const uint8_t *const *pre_density = nullptr) {
    if (!ctx || !cs || !out) return FK_ERR_BAD_ARG;
    *out = nullptr;
    SpmvPlan p(cs, copies, pre_cidx, pre_table, n_pre_table, pre_density, ctx->err);
    std::unique_ptr<fk_r1cs_dev> r(new fk_r1cs_dev());
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    FK_TRY(plan_validate(p, *r));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_load0 = std::chrono::steady_clock::now();
    double t_copy = 0;
    FK_TRY(plan_class_lists(p, *r));
    for (int k = 0; k < 3; k++) {
        FK_TRY(plan_coefficients(p, *r, k));
        const uint64_t nnz = p.ptr[k][p.ng];
        const auto tc0 = std::chrono::steady_clock::now();
        FK_TRY(dev_upload(ctx, r->ptr[k], p.ptr[k], p.ng + 1));
        FK_TRY(dev_upload(ctx, r->col[k], p.col[k], nnz, 1));
        FK_TRY(dev_upload(ctx, r->cidx[k], p.trusted() ? pre_cidx[k] : p.cidx[k].data(), nnz, 1));
        t_copy += since(tc0);
        if (pre_cidx || !p.want_alias) std::vector<uint32_t>().swap(p.cidx[k]);
        if (!r->h_rowlist[k].empty()) FK_TRY(dev_upload(ctx, r->rowlist[k], r->h_rowlist[k].data(), r->h_rowlist[k].size()));
        r->bins.rowlist[k] = r->rowlist[k];
    }
    if (getenv("FK_GATES_TRACE")) fprintf(stderr, "[fk] r1cs load: %.2f s so far, %.2f of them allocating and copying the matrices\n", since(t_load0), t_copy);
    plan_windows(p, *r);
    FK_TRY(window_need(ctx, p, *r));
    FK_TRY(plan_aliases(p, *r));
    FK_TRY(plan_dedup(p, *r));
    for (int k = 0; k < 3 && r->n_alias; k++) {       // bins_dd points at the full list of a matrix that has no alias
        if (!p.is_alias[k].empty()) FK_TRY(dev_upload(ctx, r->rowlist_dd[k], p.dd[k].data(), p.dd[k].size(), 1));
        r->bins_dd.rowlist[k] = p.is_alias[k].empty() ? r->rowlist[k].p : r->rowlist_dd[k].p;
    }
    if (r->n_alias) FK_TRY(dev_upload(ctx, r->d_alias, p.alias.data(), p.alias.size()));
    std::vector<uint64_t>().swap(p.alias); for (int k = 0; k < 3; k++) { std::vector<uint32_t>().swap(p.dd[k]); std::vector<uint8_t>().swap(p.is_alias[k]); }
    if (getenv("FK_GATES_TRACE") && p.want_alias && r->bins.mask) fprintf(stderr, "[fk] r1cs load: %.2f s so far, alias plan done (%llu aliases for %llu terms)\n", since(t_load0),
                                                         (unsigned long long)r->n_alias, (unsigned long long)r->alias_terms);
    plan_wavelist(p, *r);
    if (r->n_wavelist) FK_TRY(dev_upload(ctx, r->d_wavelist, p.wavelist.data(), p.wavelist.size()));
    plan_queries(p, *r);
    FK_TRY(dev_upload(ctx, r->table, p.table.data(), p.table.size()));
    for (auto m : {std::make_pair(&r->d_a_aux, &p.a_aux), std::make_pair(&r->d_b_in, &p.b_in), std::make_pair(&r->d_b_aux, &p.b_aux)}) FK_TRY(dev_upload(ctx, *m.first, m.second->data(), m.second->size()));
    FK_TRY(dev_upload(ctx, r->d_idx_a, p.idx_a.data(), p.idx_a.size(), 1));
    FK_TRY(dev_upload(ctx, r->d_idx_b, p.idx_b.data(), p.idx_b.size(), 1));
    r->qidx.a = r->d_idx_a; r->qidx.b = r->d_idx_b; r->qidx.n_a = p.idx_a.size(); r->qidx.n_b = p.idx_b.size();
    // what a key's padded A array (msm.hip: key_a_pad) is cached under: which aux variables the A query takes
    FK_TRY(query_fingerprint(ctx, r->d_idx_a, p.idx_a.size(), &r->qidx.a_fp));
    r->qidx.a_fp_valid = true;
    *out = r.release();
    return FK_OK;
}

int r1cs_load_coded(fk_ctx *ctx, uint32_t num_input, uint32_t num_aux, uint64_t num_gates, const uint64_t *const ptr[3], const uint32_t *const col[3],
                    const uint32_t *const cidx[3], const Fr *table, uint64_t n_table, fk_r1cs_dev **out, const uint8_t *const density[3]) {
    fk_r1cs cs{};
    cs.num_input = num_input; cs.num_aux = num_aux; cs.num_gates = num_gates;
    cs.a_ptr = ptr[0]; cs.a_col = col[0]; cs.b_ptr = ptr[1]; cs.b_col = col[1]; cs.c_ptr = ptr[2]; cs.c_col = col[2];
    return r1cs_load_impl(ctx, &cs, 1, out, cidx, table, n_table, density);
}

}  // namespace fk

using namespace fk;

extern "C" {

void fk_r1cs_free(fk_ctx *ctx, fk_r1cs_dev *r) {
    if (!r) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete r;
}

int fk_r1cs_load(fk_ctx *ctx, const fk_r1cs *cs, fk_r1cs_dev **out) { return fk_guard(ctx, [&]() -> int { return r1cs_load_impl(ctx, cs, 1, out); }); }
int fk_r1cs_load_tiled(fk_ctx *ctx, const fk_r1cs *instance, uint32_t copies, fk_r1cs_dev **out) { return fk_guard(ctx, [&]() -> int { return r1cs_load_impl(ctx, instance, copies, out); }); }

// the same system with its coefficients already dictionary-coded by the caller: *_val of `cs` are ignored, cidx[k][i] indexes
// `table` (n_table Montgomery values, table[0] = ONE).  8 bytes per term on the host side as well -- how a system of 10^9
// explicit terms is handed over (32-byte values per term would be 30 GB of host memory).
int fk_r1cs_load_coded(fk_ctx *ctx, const fk_r1cs *cs, const uint32_t *a_cidx, const uint32_t *b_cidx, const uint32_t *c_cidx, const uint64_t *table,
                       uint64_t n_table, fk_r1cs_dev **out) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!cs || !table || !n_table || !out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs: null argument");
    const uint32_t *cidx[3] = {a_cidx, b_cidx, c_cidx};
    return r1cs_load_impl(ctx, cs, 1, out, cidx, (const Fr *)table, n_table);
}); }

int fk_r1cs_density_ptrs(const fk_r1cs_dev *r, const void *out[3]) {
    if (!r || !out) return FK_ERR_BAD_ARG;
    out[0] = r->d_a_aux; out[1] = r->d_b_in; out[2] = r->d_b_aux;
    return FK_OK;
}

int fk_r1cs_info(const fk_r1cs_dev *r, uint64_t out[8]) {
    if (!r || !out) return FK_ERR_BAD_ARG;
    const uint64_t v[8] = {r->num_gates + r->num_input, r->nnz[0], r->nnz[1], r->nnz[2], r->n_table,
                           (uint64_t)r->num_input + r->n_a_aux, r->n_b_in + r->n_b_aux, (uint64_t)r->num_input + r->num_aux};
    memcpy(out, v, sizeof v);
    return FK_OK;
}

// inspection for the tests: the alias plan of a resident system (r1cs.hpp)
int fk_r1cs_alias_info(const fk_r1cs_dev *r, uint64_t out[4]) {
    if (!r || !out) return FK_ERR_BAD_ARG;
    out[0] = r->n_alias; out[1] = r->n_alias ? r->alias_terms : 0; out[2] = r->alias_min; out[3] = r->alias_lookback;
    return FK_OK;
}

static void alias_unpack(uint64_t e, uint32_t *dst_mtx, uint32_t *dst_row, uint32_t *src_mtx, uint32_t *src_row) {
    *dst_row = (uint32_t)e; *src_row = (uint32_t)e - ((uint32_t)(e >> 32) & 0xffffu);
    *dst_mtx = (uint32_t)(e >> 48) & 3u; *src_mtx = (uint32_t)(e >> 50) & 3u;
}
int fk_r1cs_aliases(const fk_r1cs_dev *r, uint64_t cap, uint32_t *dst_mtx, uint32_t *dst_row, uint32_t *src_mtx, uint32_t *src_row) {
    if (!r || !dst_mtx || !dst_row || !src_mtx || !src_row || cap < r->n_alias) return FK_ERR_BAD_ARG;
    if (!r->n_alias) return FK_OK;
    try {
        std::vector<uint64_t> h(r->n_alias);
        if (hipMemcpy(h.data(), r->d_alias, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return FK_ERR_HIP;
        for (uint64_t i = 0; i < h.size(); i++) alias_unpack(h[i], &dst_mtx[i], &dst_row[i], &src_mtx[i], &src_row[i]);
    } catch (...) { return FK_ERR_OOM; }
    return FK_OK;
}

int fk_r1cs_windows(const fk_r1cs_dev *r, uint32_t *n_windows, uint64_t rows[17], uint64_t need[16]) {
    if (!r || !n_windows) return FK_ERR_BAD_ARG;
    *n_windows = r->win_k;
    for (uint32_t j = 0; j <= r->win_k && rows; j++) rows[j] = r->win_row[j];
    for (uint32_t j = 0; j < r->win_k && need; j++) need[j] = r->win_need[j];
    return FK_OK;
}

// inspection for the tests: the loader's stages (spmv_plan.hpp) in the loader's order, without its uploads; host only
static void plan_segs_out(const BinArgs &b, fk_r1cs_plan_segs *o) {
    static_assert(FK_PLAN_SEGS == SPMV_SEGS && FK_PLAN_WIN_MAX == fk_r1cs_dev::WIN_MAX, "fawkes_hip_inspect.h mirrors r1cs.hpp");
    o->nseg = b.nseg; o->mask = b.mask;
    memcpy(o->mtx, b.mtx, sizeof b.mtx); memcpy(o->lg, b.lg, sizeof b.lg); memcpy(o->rows, b.n_rows, sizeof b.n_rows);
    memcpy(o->list_off, b.list_off, sizeof b.list_off); memcpy(o->first_block, b.first_block, sizeof b.first_block);
}
int fk_r1cs_plan_host(const fk_r1cs *cs, uint32_t copies, const uint32_t *a_cidx, const uint32_t *b_cidx, const uint32_t *c_cidx, const uint64_t *table,
                      uint64_t n_table, fk_r1cs_plan_info *out) { return fk_guard((fk_ctx *)nullptr, [&]() -> int {
    if (!cs || !out) return FK_ERR_BAD_ARG;
    const uint32_t *cidx[3] = {a_cidx, b_cidx, c_cidx};
    const bool coded = a_cidx || b_cidx || c_cidx || table;
    SpmvPlan p(cs, copies, coded ? cidx : nullptr, (const Fr *)table, n_table, nullptr, tls_error());
    fk_r1cs_dev r;           // its plain fields and h_rowlist; no device array is ever allocated
    FK_TRY(plan_validate(p, r));
    FK_TRY(plan_class_lists(p, r));
    for (int k = 0; k < 3; k++) FK_TRY(plan_coefficients(p, r, k));
    plan_windows(p, r);
    FK_TRY(plan_aliases(p, r));
    FK_TRY(plan_dedup(p, r));
    plan_wavelist(p, r);
    plan_queries(p, r);
    auto put = [](uint32_t *dst, const std::vector<uint32_t> &v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * 4); };
    plan_segs_out(r.bins, &out->segs); plan_segs_out(r.bins_dd, &out->segs_dd);
    for (int k = 0; k < 3; k++) {
        put(out->list[k], r.h_rowlist[k]); put(out->list_dd[k], p.dd[k]);
        out->own_dd[k] = !p.is_alias[k].empty(); out->n_dd[k] = (uint32_t)p.dd[k].size();
        out->wave_from[k] = r.wave_from[k]; out->wave_to[k] = r.wave_to[k];
    }
    for (uint64_t i = 0; i < p.alias.size() && out->alias_dst_mtx && out->alias_dst_row && out->alias_src_mtx && out->alias_src_row; i++)
        alias_unpack(p.alias[i], &out->alias_dst_mtx[i], &out->alias_dst_row[i], &out->alias_src_mtx[i], &out->alias_src_row[i]);
    put(out->idx_a, p.idx_a); put(out->idx_b, p.idx_b);
    out->win_k = r.win_k;
    memcpy(out->win_row, r.win_row, sizeof r.win_row); memcpy(out->win_alias, r.win_alias, sizeof r.win_alias);
    memcpy(out->win_cnt, r.win_cnt, sizeof r.win_cnt); memcpy(out->win_cnt_dd, r.win_cnt_dd, sizeof r.win_cnt_dd);
    out->n_alias = r.n_alias; out->alias_terms = r.n_alias ? r.alias_terms : 0; out->alias_min = r.alias_min; out->alias_lookback = r.alias_lookback;
    out->n_idx_a = p.idx_a.size(); out->n_idx_b = p.idx_b.size();
    return FK_OK;
}); }

}  // extern "C"
namespace fk {
// The per-log_w residue-grouped class lists of a constraint system with binned matrices (see SliceLists), built on first use.
static int slice_lists(fk_ctx *ctx, const fk_r1cs_dev *r, uint32_t log_w, const SliceLists **out) {
    std::lock_guard<std::mutex> lock(r->slice_mu);
    SliceLists &sl = r->slices[log_w];
    if (!sl.built) {
        const uint32_t W = 1u << log_w;
        for (int k = 0; k < 3; k++) {
            if (!((r->bins.mask >> k) & 1)) continue;
            const std::vector<uint32_t> &src = r->h_rowlist[k];
            std::vector<uint32_t> dst(src.size());
            for (uint32_t s = 0; s < r->bins.nseg; s++) {
                if (r->bins.mtx[s] != (uint32_t)k) continue;
                const uint32_t off = r->bins.list_off[s], nr = r->bins.n_rows[s];
                uint32_t c[8] = {0};
                for (uint32_t i = 0; i < nr; i++) c[src[off + i] & (W - 1)]++;
                uint32_t pos[8], acc = 0;
                for (uint32_t q = 0; q < W; q++) { sl.cnt[s][q] = c[q]; sl.offs[s][q] = acc; pos[q] = acc; acc += c[q]; }
                for (uint32_t i = 0; i < nr; i++) { const uint32_t row = src[off + i]; dst[off + pos[row & (W - 1)]++] = row; }   // stable: longest first inside a group
            }
            FK_TRY(dev_upload(ctx, sl.d_list[k], dst.data(), dst.size(), 1));        // (a call that fails here leaves built false: the next one allocates afresh)
        }
        sl.built = true;
    }
    *out = &sl;
    return FK_OK;
}

// a, b, c <- the rows t = rank (mod 2^log_w) of A z, B z, C z, densely: out[j] = row rank + j * 2^log_w (sliced), or all rows
// (not sliced: rank = log_w = 0).  n_out: elements the caller's arrays hold; those behind the last row are zeroed when sliced.
int r1cs_eval_impl(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, void *d_a, void *d_b, void *d_c, bool sliced, uint32_t rank, uint32_t log_w, uint64_t n_out, int window = -1) {
    FK_HIP(ctx, hipSetDevice(ctx->device));
    SpmvArgs a;
    for (int k = 0; k < 3; k++) { a.ptr[k] = r->ptr[k]; a.col[k] = r->col[k]; a.cidx[k] = r->cidx[k]; }
    a.out[0] = (Fr *)d_a; a.out[1] = (Fr *)d_b; a.out[2] = (Fr *)d_c;
    const uint64_t rows = r->num_gates + r->num_input;
    const uint64_t W = (uint64_t)1 << log_w;
    const uint64_t my_rows = sliced ? (rows > rank ? (rows - rank + W - 1) / W : 0) : rows;      // row groups this launch evaluates
    if (sliced) {
        if (my_rows > n_out) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs eval: the slice holds %llu rows, the arrays %llu", (unsigned long long)my_rows, (unsigned long long)n_out);
        if (n_out > my_rows) for (int k = 0; k < 3; k++) FK_HIP(ctx, hipMemsetAsync(a.out[k] + my_rows, 0, (n_out - my_rows) * sizeof(Fr), ctx->stream));
    }
    // lanes per row: half of the matrix's mean row length, rounded down to a power of two (1 .. 64); measured on the eddsa batch: 16 / 8 / 4 / 2 / 1 terms per lane -> 1.51 / 1.27 / 1.16 / 1.02 / 0.97 ms
    uint32_t lg[3], lgmax = 0;
    static const int t_div = std::max(1, tune("FK_SPMV_TERMS_PER_LANE", 2));
    for (int k = 0; k < 3; k++) {
        const uint64_t mean = r->num_gates ? r->nnz[k] / r->num_gates : 0;
        lg[k] = 0;
        while (!((r->bins.mask >> k) & 1) && lg[k] < 6 && ((uint64_t)t_div << lg[k]) <= mean) lg[k]++;
        if (lg[k] > lgmax) lgmax = lg[k];
    }
    const uint64_t lanes = my_rows << lgmax;
    const TileDims td{r->base_gates, r->base_input, r->base_aux};
    const uint32_t binned = r->bins.mask;
    const dim3 grid((unsigned)((lanes + 255) / 256), 3), block(256);
    const bool tiled = r->copies > 1;
    // window >= 0 (explicit system, every matrix binned): only the class-list entries of row window `window`; the rows behind the gates
    // (this kernel's only work then) go with window 0
    if (lanes && window <= 0) {
#define FK_SPMV_LAUNCH(T_, S_) hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_kernel<T_, S_>), grid, block, 0, ctx->stream, a, r->table, (const Fr *)d_z, r->num_gates, \
                                                  r->num_input, lg[0], lg[1], lg[2], td, binned, log_w, rank)
        if (tiled) { if (sliced) FK_SPMV_LAUNCH(true, true); else FK_SPMV_LAUNCH(true, false); }
        else { if (sliced) FK_SPMV_LAUNCH(false, true); else FK_SPMV_LAUNCH(false, false); }
#undef FK_SPMV_LAUNCH
    }
    // explicit system, unsliced: the class lists without the alias rows, then the aliases copied from their sources (r1cs.hpp)
    const bool dedup = r->n_alias && !tiled && !sliced && spmv_dedup_on();
    if (binned) {
        BinArgs b = dedup ? r->bins_dd : r->bins;
        SliceArgs sa;
        if (sliced) {
            // this rank's plan: copy c needs the rows = rank - c * base_gates (mod W); the residues repeat every P copies
            const SliceLists *sl = nullptr;
            FK_TRY(slice_lists(ctx, r, log_w, &sl));
            sa.log_w = log_w; sa.rank = rank;
            const uint32_t g = (uint32_t)(r->base_gates & (W - 1));
            uint32_t P = 1;
            while ((uint32_t)((uint64_t)P * g) & (W - 1)) P++;
            sa.P = P;
            for (uint32_t p_ = 0; p_ < P; p_++) sa.rho[p_] = (uint32_t)((rank + W * P - ((uint64_t)p_ * g & (W - 1))) & (W - 1));
            for (uint32_t s = 0; s < b.nseg; s++) {
                memcpy(sa.cnt[s], sl->cnt[s], sizeof sa.cnt[s]); memcpy(sa.offs[s], sl->offs[s], sizeof sa.offs[s]);
                uint64_t T = 0, part = 0;
                const uint32_t tail = r->copies % P;
                for (uint32_t p_ = 0; p_ < P; p_++) { T += sa.cnt[s][sa.rho[p_]]; if (p_ < tail) part += sa.cnt[s][sa.rho[p_]]; }
                sa.T[s] = (uint32_t)T;
                FK_TRY(bin_segment(ctx->err, b, s, b.mtx[s], b.lg[s], b.list_off[s], b.n_rows[s], (uint64_t)(r->copies / P) * T + part));
            }
            for (int k = 0; k < 3; k++) b.rowlist[k] = sl->d_list[k];
        }
        if (tiled && !sliced && r->n_wavelist) {
            // rows of wave_lo .. wave_hi - 1 terms go to spmv_tiled_wave_kernel: they are rowlist[wave_from, wave_to) of their matrix
            // (the lists are sorted by length, longest first), i.e. with the default [4, 64): the whole 8-, 4- and 2-lane classes and the
            // 4 .. 7-term head of the one-lane class; with wave_hi > 64 also the tail of the 16-lane class
            for (uint32_t s = 0; s < b.nseg; s++) {
                const uint32_t k = b.mtx[s], s0 = b.list_off[s], s1 = s0 + b.n_rows[s], w0 = r->wave_from[k], w1 = r->wave_to[k];
                uint32_t lo = s0, hi = s1;
                if (w0 <= s0) lo = std::min(std::max(s0, w1), s1); else hi = std::min(s1, w0);      // (load keeps the wave range from lying strictly inside a class)
                FK_TRY(bin_segment(ctx->err, b, s, k, b.lg[s], lo, hi - lo, (uint64_t)(hi - lo) * r->copies));
            }
            const uint64_t n_waves = (uint64_t)((r->copies + 63) / 64) * r->n_wavelist;
            hipLaunchKernelGGL(spmv_tiled_wave_kernel, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, ctx->stream, a, r->table, (const Fr *)d_z, r->num_input, td,
                               r->copies, r->d_wavelist, r->n_wavelist, (uint32_t)n_waves);
        }
        if (window >= 0) {
            for (uint32_t s = 0; s < b.nseg; s++) {
                const uint32_t c0 = (dedup ? r->win_cnt_dd : r->win_cnt)[window][s], c1 = (dedup ? r->win_cnt_dd : r->win_cnt)[window + 1][s];
                FK_TRY(bin_segment(ctx->err, b, s, b.mtx[s], b.lg[s], b.list_off[s] + c0, c1 - c0, c1 - c0));
            }
        }
        const unsigned blocks = b.first_block[b.nseg];
        if (blocks) {
#define FK_SPMVB_LAUNCH(T_, S_) hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_binned_kernel<T_, S_>), dim3(blocks), dim3(256), 0, ctx->stream, a, b, r->table, (const Fr *)d_z, \
                                                   r->num_input, td, r->copies, sa)
            if (tiled) { if (sliced) FK_SPMVB_LAUNCH(true, true); else FK_SPMVB_LAUNCH(true, false); }
            else { if (sliced) FK_SPMVB_LAUNCH(false, true); else FK_SPMVB_LAUNCH(false, false); }
#undef FK_SPMVB_LAUNCH
        }
        if (dedup) {
            const uint64_t a0 = window >= 0 ? r->win_alias[window] : 0, a1 = window >= 0 ? r->win_alias[window + 1] : r->n_alias;      // dst in this window: src in it or an earlier one
            if (a1 > a0) hipLaunchKernelGGL(spmv_alias_kernel, dim3((unsigned)((a1 - a0 + 255) / 256)), dim3(256), 0, ctx->stream, a.out[0], a.out[1], a.out[2], r->d_alias + a0, a1 - a0);
        }
    }
    FK_HIP(ctx, hipGetLastError());
    FK_DBG(ctx, "spmv");
    return FK_OK;
}
}  // namespace fk
extern "C" {

// a, b, c: device arrays with room for next_pow2(rows) elements each (fk_prove_dev's contract); rows written.
int fk_r1cs_eval_dev(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, void *d_a, void *d_b, void *d_c) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!r || !d_z || !d_a || !d_b || !d_c) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs eval: null argument");
    return r1cs_eval_impl(ctx, r, d_z, d_a, d_b, d_c, false, 0, 0, 0);
}); }

// Multi-GPU form: only the cyclic slice rank `rank` of 2^log_w ranks needs -- local[j] = row (rank + j * 2^log_w) of A z, B z,
// C z, zero behind the last row: exactly what fk_dq_gather_dev would cut out of the full vectors, at 1 / 2^log_w of the work and
// without the three m-element vectors.  Arrays of 2^(log_m - log_w) elements.
int fk_r1cs_eval_slice_dev(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, uint32_t log_m, uint32_t rank, uint32_t log_w, void *d_a, void *d_b, void *d_c) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!r || !d_z || !d_a || !d_b || !d_c) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs eval: null argument");
    if (log_w > 3 || (rank >> log_w) || log_m < log_w || log_m >= FK_FR_S) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs eval: bad slice (rank %u of 2^%u, domain 2^%u)", rank, log_w, log_m);
    if (r->num_gates + r->num_input > ((uint64_t)1 << log_m)) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "r1cs eval: the system has more rows than the domain 2^%u", log_m);
    return r1cs_eval_impl(ctx, r, d_z, d_a, d_b, d_c, true, rank, log_w, (uint64_t)1 << (log_m - log_w));
}); }

}  // extern "C"
namespace fk {
// The body of fk_prove_r1cs_dev, shared with fk_prove_r1cs_checked_dev (check.hip) and fk_prove_r1cs_wait.  after_eval (may be null): called
// once the evaluation of a, b, c into the stage buffers is queued on the main stream and before the quotient that consumes them is; what it
// queues there reads the very a, b, c the proof is made from.  An entry that passes one does not join the submit / wait pipeline: any
// outstanding early front is refused.  before_block (may be null): ProveRun's.
int prove_r1cs_dev_impl(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_z, const uint64_t rr[4], const uint64_t ss[4],
                        uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm, const std::function<int()> *after_eval, const std::function<int()> *before_block) {
    if (!key || !r || !d_z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: null argument");
    uint64_t rows = 0;
    FK_TRY(r1cs_fits_key(ctx, r, key, &rows));
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t mb = key->m * sizeof(Fr);
    if (after_eval && ctx->early.done) { msm_abandon(ctx); FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: an early front of a submitted proof is outstanding"); }
    ProveRun run{r1cs_queries(r), false, before_block};      // the queries' index lists are known: no per-proof density compaction
    if (ctx->early.done && ctx->early.key == key && ctx->early.r1cs == r && ctx->early.d_z == d_z) {
        // the front of this proof -- ev_z, the evaluation of a, b, c into the stage buffers, the witness multiplications' sorts --
        // was queued while the previous proof's tails ran (early_front below): go on with the quotient
        run.z_recorded = true;
    } else {
        if (ctx->early.done) { msm_abandon(ctx); FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: an early front of another proof is outstanding"); }
        FK_HIP(ctx, ctx->stage_a.reserve(mb)); FK_HIP(ctx, ctx->stage_b.reserve(mb)); FK_HIP(ctx, ctx->stage_c.reserve(mb));
        // z is complete at this point of the main stream: the witness multiplications wait for THIS, not for the evaluation of a, b, c
        // (11.6 ms at 2^25 during which nothing else ran; FK_PROVE_Z_EARLY=0 restores that)
        static const int t_zearly = tune("FK_PROVE_Z_EARLY", 1);
        if (t_zearly) {
            FK_HIP(ctx, hipEventRecord(ctx->ev_z, ctx->stream));
            run.z_recorded = true;
        }
        FK_TRY(fk_r1cs_eval_dev(ctx, r, d_z, ctx->stage_a.p, ctx->stage_b.p, ctx->stage_c.p));
        if (after_eval) FK_TRY((*after_eval)());
    }
    return prove_dev(ctx, key, ctx->stage_a.as<Fr>(), ctx->stage_b.as<Fr>(), ctx->stage_c.as<Fr>(), rows, (const Fr *)d_z, run, rr, ss, out_proof, tm);
}
}  // namespace fk
extern "C" {

// witness in -> proof out: SpMV, quotient, MSMs, assembly.  z: device pointer (num_input + num_aux elements).
int fk_prove_r1cs_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_z, const uint64_t rr[4], const uint64_t ss[4],
                      uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_r1cs_dev");
    if (!ctx) return FK_ERR_BAD_ARG;
    return prove_r1cs_dev_impl(ctx, key, r, d_z, rr, ss, out_proof, tm, nullptr, nullptr);
}); }

// multi-GPU: all five multiplications of this key's slices for a resident constraint system (see fk_prove_msms_hz_dev)
int fk_prove_msms_hz_r1cs_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_h_slice, const void *d_z,
                              uint8_t out[FK_MSM_RESULT_BYTES]) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!key || !r || !d_z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: null argument");
    FK_TRY(r1cs_fits_key(ctx, r, key, nullptr));
    FK_TRY(witness_queries_begin(ctx, key, d_z, r1cs_queries(r)));
    return witness_queries_finish(ctx, key, d_h_slice, out);
}); }

// ... and of fk_prove_msms_z_begin_dev: the witness multiplications are queued (index-list gathers), the caller runs the
// (distributed) quotient and finishes with fk_prove_msms_finish_dev
int fk_prove_msms_z_begin_r1cs_dev(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_z) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!key || !r || !d_z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: null argument");
    FK_TRY(r1cs_fits_key(ctx, r, key, nullptr));
    return witness_queries_begin(ctx, key, d_z, r1cs_queries(r));
}); }

}  // extern "C"
namespace fk {
// ONE proof at a time from a witness in host memory, with the hand-over CHUNKED (round 5): the 1.07 GB upload of the benchmark's witness is
// 19 ms during which nothing else of this proof could run -- the proof's latency was upload + proof.  A circuit's rows read the variables
// allocated before them, so the rows below win_row[j + 1] need only the first win_need[j] elements of z (planned at load, r1cs.hpp): the
// witness goes up in win_k pieces on the copy stream and the evaluation of window j is queued behind piece j -- a, b, c are complete ~2 ms after
// the last byte has landed instead of ~20 ms, and the witness sorts then run without the evaluation beside them.  A system whose first rows
// read late variables degenerates to "upload everything, then evaluate" (win_need[0] = all of z).  Same kernels, same row order inside a
// window, same bytes.
static int prove_r1cs_chunked(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, uint64_t rows, const uint64_t *z, const uint64_t rr[4], const uint64_t ss[4],
                              uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm) {
    const size_t mb = key->m * sizeof(Fr);
    FK_HIP(ctx, ctx->stage_a.reserve(mb)); FK_HIP(ctx, ctx->stage_b.reserve(mb)); FK_HIP(ctx, ctx->stage_c.reserve(mb));
    // the pieces follow whatever the main stream still has queued (stage_z may be read by it)
    FK_HIP(ctx, hipEventRecord(ctx->ev_upload_gate, ctx->stream));
    FK_HIP(ctx, hipStreamWaitEvent(ctx->copy_st, ctx->ev_upload_gate, 0));
    Fr *d_z = ctx->stage_z.as<Fr>();
    uint64_t off = 0;
    ProveRun run{r1cs_queries(r)};
    int rc = FK_OK;
    // piece j, then window j: from pageable memory hipMemcpyAsync returns only when the piece has been staged, so the windows must be
    // queued BETWEEN the pieces for the evaluation to run beside the rest of the upload
    for (uint32_t j = 0; j < r->win_k && rc == FK_OK; j++) {
        const uint64_t end = r->win_need[j];
        hipError_t e = hipSuccess;
        if (end > off) e = hipMemcpyAsync(d_z + off, z + 4 * off, (end - off) * sizeof(Fr), hipMemcpyHostToDevice, ctx->copy_st);
        if (e == hipSuccess && !ctx->ev_chunk[j]) e = hipEventCreateWithFlags(&ctx->ev_chunk[j], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_chunk[j], ctx->copy_st);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_chunk[j], 0);
        off = std::max(off, end);
        if (e == hipSuccess && j + 1 == r->win_k) {        // z is complete at this point of the main stream: the witness multiplications wait for THIS, not for the last window
            e = hipEventRecord(ctx->ev_z, ctx->stream);
            run.z_recorded = e == hipSuccess;
        }
        if (e != hipSuccess) { rc = FK_ERR_HIP; ctx->err = std::string("prove: chunked hand-over: ") + hipGetErrorString(e); break; }
        rc = r1cs_eval_impl(ctx, r, d_z, ctx->stage_a.p, ctx->stage_b.p, ctx->stage_c.p, false, 0, 0, 0, (int)j);
    }
    if (rc == FK_OK) return prove_dev(ctx, key, ctx->stage_a.as<Fr>(), ctx->stage_b.as<Fr>(), ctx->stage_c.as<Fr>(), rows, d_z, run, rr, ss, out_proof, tm);
    (void)hipStreamSynchronize(ctx->copy_st); (void)hipStreamSynchronize(ctx->stream);        // the caller's buffer is no longer read when an error returns
    return rc;
}
}  // namespace fk
extern "C" {

int fk_prove_r1cs(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const uint64_t *z, const uint64_t rr[4], const uint64_t ss[4],
                  uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_r1cs");
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!key || !r || !z) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: null argument");
    FK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t zb = ((size_t)r->num_input + r->num_aux) * sizeof(Fr);
    FK_HIP(ctx, ctx->stage_z.reserve(zb));
    static const bool t_chunked = !(getenv("FK_PROVE_CHUNKED_UPLOAD") && atoi(getenv("FK_PROVE_CHUNKED_UPLOAD")) == 0);      // documented switch (fawkes_hip.h)
    if (t_chunked && r->win_k >= 2 && !ctx->early.done && !ctx->wslot[0].pending && !ctx->wslot[1].pending) {
        uint64_t rows = 0;
        FK_TRY(r1cs_fits_key(ctx, r, key, &rows));
        return prove_r1cs_chunked(ctx, key, r, rows, z, rr, ss, out_proof, tm);
    }
    FK_HIP(ctx, hipMemcpyAsync(ctx->stage_z.p, z, zb, hipMemcpyHostToDevice, ctx->stream));
    return fk_prove_r1cs_dev(ctx, key, r, ctx->stage_z.p, rr, ss, out_proof, tm);
}); }

// Pipelined form of fk_prove_r1cs: _submit starts the upload of the witness into one of the two slots and returns at once;
// _wait computes that proof.  Calling submit(k+1) before wait(k) hides the upload of proof k+1 underneath proof k.
int fk_prove_r1cs_submit(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const uint64_t *z, const uint64_t rr[4], const uint64_t ss[4], int *ticket) { return fk_guard(ctx, [&]() -> int {
    if (!ctx) return FK_ERR_BAD_ARG;
    if (!key || !r || !z || !rr || !ss || !ticket) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: null argument");
    const int slot = ctx->wslot_next;
    if (ctx->wslot[slot].pending) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: two proofs are already submitted (call fk_prove_r1cs_wait first)");
    fk_ctx::WitSlot &w = ctx->wslot[slot];
    const size_t zb = ((size_t)r->num_input + r->num_aux) * sizeof(Fr);
    // With another proof submitted ahead of this one, the upload is left to THAT proof's run: it queues the copy behind its
    // memory-bound front (sorts, evaluation of a, b, c), so that the transfer runs underneath transforms and accumulations.
    // Started here it ran beside the sorts: +14 ms per proof on the synthetic 2^25 shape (1 GiB witness), +0.8 ms on the
    // 1024-transaction system (profiles/r02_sorts_first_probe.log).  FK_UPLOAD_DEFER=0: start it here.  The host buffer must
    // stay valid until fk_prove_r1cs_wait(ticket) returns either way.
    static const int t_defer = tune("FK_UPLOAD_DEFER", 1);
    if (t_defer && ctx->wslot[slot ^ 1].pending && zb <= w.buf.cap && w.ready) { w.deferred = true; w.host_z = z; w.host_bytes = zb; }
    else { w.deferred = false; FK_TRY(fk_witness_upload_async(ctx, slot, z, zb)); }
    w.pending = true; w.key = key; w.r1cs = r;
    memcpy(w.r, rr, 32); memcpy(w.s, ss, 32);
    ctx->wslot_next = slot ^ 1;
    *ticket = slot;
    return FK_OK;
}); }
}  // extern "C"
namespace fk {
// Early front of the proof waiting in witness slot `slot` (pipelined proofs at sizes that run the sorts-first schedule): called by
// the prover when everything of the CURRENT proof is queued.  The current proof ends on latency-bound tails -- G2's bucket
// reduction behind H's accumulation: ~7 ms at 2^25 during which the GPU is mostly idle -- and the next proof begins with
// memory-bound work that needs nothing from it: the evaluation of a, b, c and the witness multiplications' sorts.  They are queued
// here behind the current proof's LAST ACCUMULATION (underneath an accumulation they would only take its time, csrc/prover.hip),
// so they fill that idle stretch and the host's turnaround between two proofs.
static int early_front(fk_ctx *ctx, int slot) {
    fk_ctx::WitSlot &w = ctx->wslot[slot];
    const fk_key *key = w.key; const fk_r1cs_dev *r = w.r1cs;
    if (w.deferred) { w.deferred = false; FK_TRY(fk_witness_upload_async(ctx, slot, w.host_z, w.host_bytes)); }
    void *d_z = nullptr;
    FK_TRY(fk_witness_ptr(ctx, slot, &d_z));               // the main stream waits for the slot's upload
    if (ctx->ev_acc_done_valid) FK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_acc_done, 0));      // ... and for the current proof's last accumulation (H's)
    const size_t mb = key->m * sizeof(Fr);
    if (mb > ctx->stage_a.cap || mb > ctx->stage_b.cap || mb > ctx->stage_c.cap) return FK_OK;       // never grow buffers the current proof may still read: no early front
    FK_HIP(ctx, hipEventRecord(ctx->ev_z, ctx->stream));
    int tails[5];
    const int wb = early_witness_begin(ctx, key, d_z, r1cs_queries(r), tails);
    if (wb < 0) return -wb;
    if (wb == 0) return FK_OK;     // (the schedule does not apply: nothing was queued but the waits)
    FK_TRY(fk_r1cs_eval_dev(ctx, r, d_z, ctx->stage_a.p, ctx->stage_b.p, ctx->stage_c.p));
    ctx->early.done = true; ctx->early.key = key; ctx->early.r1cs = r; ctx->early.d_z = d_z;
    memcpy(ctx->early.tails, tails, sizeof tails);
    return FK_OK;
}
}  // namespace fk
extern "C" {
int fk_prove_r1cs_wait(fk_ctx *ctx, int ticket, uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm) { return fk_guard(ctx, [&]() -> int {
    FK_RANGE("fk_prove_r1cs_wait");
    if (!ctx) return FK_ERR_BAD_ARG;
    if (ticket < 0 || ticket > 1 || !ctx->wslot[ticket].pending) FK_SET_ERR(ctx, FK_ERR_BAD_ARG, "prove: no submitted proof with ticket %d", ticket);
    fk_ctx::WitSlot &w = ctx->wslot[ticket];
    w.pending = false;
    if (w.deferred) { w.deferred = false; FK_TRY(fk_witness_upload_async(ctx, ticket, w.host_z, w.host_bytes)); }      // nobody ran in between
    void *d_z = nullptr;
    const bool early = ctx->early.done && ctx->early.key == w.key && ctx->early.r1cs == w.r1cs && ctx->early.d_z == ctx->wslot[ticket].buf.p;
    if (early) d_z = ctx->wslot[ticket].buf.p;            // its front is queued already (the main stream waited for the upload there)
    else FK_TRY(fk_witness_ptr(ctx, ticket, &d_z));
    // the other slot holds the NEXT proof of the same key and system: its front goes behind this proof's last accumulation
    const fk_ctx::WitSlot &o = ctx->wslot[ticket ^ 1];
    const std::function<int()> front = [ctx, ticket]() { return early_front(ctx, ticket ^ 1); };
    const bool next = o.pending && o.key == w.key && o.r1cs == w.r1cs && early_front_applies(w.key);
    return prove_r1cs_dev_impl(ctx, w.key, w.r1cs, d_z, w.r, w.s, out_proof, tm, nullptr, next ? &front : nullptr);
}); }

}  // extern "C"
