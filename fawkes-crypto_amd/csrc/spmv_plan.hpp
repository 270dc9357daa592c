// The plan of a resident constraint system (r1cs.hpp) as host-only stages: everything the loader decides before and between its uploads,
// as functions over the caller's host arrays that fill the plain fields of the resident object.  No HIP runtime call in this file: spmv.hip's
// loader runs the stages and uploads what they leave; fk_r1cs_plan_host (include/fawkes_hip_inspect.h) runs the same stages without a GPU.
#pragma once
#include "r1cs.hpp"
#include <string.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <unordered_map>

namespace fk {

// The tuning knobs of the plan, each read once (common.hpp: tune).
// rows of [wave_lo, wave_hi) terms of a batch of >= wave_copies copies go to spmv_tiled_wave_kernel (see there).  The length
// classes are 16 lanes per row from 64 terms, 8 from 32, 4 from 16, 2 from 8, one lane below; with [4, 64) the wave kernel takes
// the WHOLE 8-, 4- and 2-lane classes and the head (4 .. 7 terms) of the one-lane class.  The clipping in r1cs_eval_impl removes a
// prefix or a suffix of a class segment, so the range may cut only the first class (wave_hi >= 64) and the last one (wave_lo < 8):
// an upper bound strictly inside a middle class is snapped down to that class's boundary (experiment builds can set any value).
static const uint32_t SPMV_WAVE_COPIES = (uint32_t)tune("FK_SPMV_WAVE_MIN_COPIES", 64), SPMV_WAVE_LO = 4;
static const uint32_t SPMV_WAVE_HI_RAW = (uint32_t)std::min(1024, std::max(32, tune("FK_SPMV_WAVE_HI", 64)));
static const uint32_t SPMV_WAVE_HI = SPMV_WAVE_HI_RAW >= 64 ? SPMV_WAVE_HI_RAW : 32u;           // 32 .. 63 -> 32: the boundary between the 8-lane and the 4-lane class
static const uint32_t SPMV_BLOCK_ROWS = (uint32_t)std::max(0, tune("FK_SPMV_BLOCK_ROWS", 4096));
static const uint32_t SPMV_WINDOWS = (uint32_t)std::min<int>(fk_r1cs_dev::WIN_MAX, std::max(0, tune("FK_SPMV_WINDOWS", 8)));
static const uint32_t SPMV_DD_MIN = (uint32_t)std::max(1, tune("FK_SPMV_DEDUP_MIN", 4)), SPMV_DD_BACK = (uint32_t)std::min(4096, std::max(0, tune("FK_SPMV_DEDUP_LOOKBACK", 8)));
// FK_SPMV_DEDUP=0 (a run-time switch, read once): no alias plan at load, the full class lists and no alias kernel in the evaluation
static inline bool spmv_dedup_on() {
    static const bool on = !(getenv("FK_SPMV_DEDUP") && atoi(getenv("FK_SPMV_DEDUP")) == 0);
    return on;
}
// classes: 16 lanes per row from 64 terms, 8 from 32, 4 from 16, 2 from 8, one lane below -- a lane then has 4 .. 7 terms
// (one or two four-term steps with a shared reduction) in every class but the last
static constexpr uint32_t SPMV_CLS_LO[SPMV_CLASSES] = {64, 32, 16, 8, 0}, SPMV_CLS_LG[SPMV_CLASSES] = {4, 3, 2, 1, 0};

// Segment s of a launch of spmv_binned_kernel: `rows` entries of matrix mtx's list from list_off on, 2^lg lanes per row, `groups` lane
// groups in all (rows x copies, or what a slice keeps of them); its blocks follow those of segment s - 1.  err: where a refusal leaves its text.
static inline int bin_segment(std::string &err, BinArgs &b, uint32_t s, uint32_t mtx, uint32_t lg, uint32_t list_off, uint32_t rows, uint64_t groups) {
    const uint64_t per = 256u >> lg, blocks = (groups + per - 1) / per, first = s ? b.first_block[s] : 0;
    if (first + blocks > 0x7fffffffull) { err = "r1cs: system too large for the binned product"; return FK_ERR_BAD_ARG; }
    b.lg[s] = lg; b.mtx[s] = mtx; b.n_rows[s] = rows; b.list_off[s] = list_off;
    b.first_block[s] = (uint32_t)first; b.first_block[s + 1] = (uint32_t)(first + blocks);
    return FK_OK;
}
// entries of an ascending-by-block list that lie below row `bound`: a prefix, since blocks of rows ascend inside a class
static inline uint32_t rows_below(const uint32_t *lo, uint32_t n, uint64_t bound) {
    return (uint32_t)(std::partition_point(lo, lo + n, [&](uint32_t row) { return row < bound; }) - lo);
}
// f(0) .. f(n - 1) side by side, on n - 1 threads and the caller (a share whose thread cannot be started runs on the caller); every thread is
// joined before this returns.  false: a share threw (an exception must not leave a thread)
template <class F>
static inline bool side_by_side(uint32_t n, F f) {
    std::atomic<bool> threw{false};
    auto guarded = [&](uint32_t t) { try { f(t); } catch (...) { threw = true; } };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n; t++) { try { pool.emplace_back(guarded, t); } catch (...) { guarded(t); } }
    guarded(0);
    for (auto &th : pool) th.join();
    return !threw;
}

// One instance as the caller handed it over -- the resident system stands for `copies` of it (1 = the system itself) -- and the host arrays the
// stages build beside the resident object's plain fields.  pre_cidx / pre_table: the coefficients already dictionary-coded (gatestream.hip:
// slot 0 = ONE), val then unused.  pre_density: a_aux / b_in / b_aux flags the caller already derived (the gate decoder does, while it parses):
// the arrays then come from this library's own decoder, which has range-checked every index -- the per-term passes are skipped (trusted).
struct SpmvPlan {
    uint64_t ng; uint32_t num_input, num_aux, copies;
    const uint64_t *ptr[3]; const uint32_t *col[3]; const uint64_t *val[3];
    const uint32_t *const *pre_cidx; const Fr *pre_table; uint64_t n_pre_table; const uint8_t *const *pre_density;
    std::string &err;                                   // a stage that refuses leaves its text here and returns the code
    const bool want_alias;                              // the alias plan reads the coefficient indices of all three matrices: the loader keeps the ones it coded itself until then
    uint32_t cls_n[3][SPMV_CLASSES] = {{0}};            // rows per class; a matrix is binned (has class lists: h_rowlist) or all of them are 0
    std::vector<Fr> table;                              // coefficient dictionary; slot 0 = ONE
    std::unordered_map<std::string, uint32_t> dict;
    std::vector<uint32_t> cidx[3];
    std::vector<uint8_t> a_aux, b_in, b_aux;            // density maps
    std::vector<uint64_t> alias;                        // the device table's entries, in (dst row, dst matrix) order
    std::vector<uint8_t> is_alias[3];                   // per gate row; empty: the matrix has no alias
    std::vector<uint32_t> dd[3];                        // the dedup lists of the matrices that have aliases
    std::vector<uint32_t> wavelist, idx_a, idx_b;
    SpmvPlan(const fk_r1cs *cs, uint32_t copies_, const uint32_t *const *pc, const Fr *pt, uint64_t npt, const uint8_t *const *pd, std::string &e)
        : ng(cs->num_gates), num_input(cs->num_input), num_aux(cs->num_aux), copies(copies_), ptr{cs->a_ptr, cs->b_ptr, cs->c_ptr}, col{cs->a_col, cs->b_col, cs->c_col},
          val{cs->a_val, cs->b_val, cs->c_val}, pre_cidx(pc), pre_table(pt), n_pre_table(npt), pre_density(pd), err(e), want_alias(copies_ == 1 && spmv_dedup_on()) {}
    bool trusted() const { return pre_density && pre_cidx; }
    uint64_t len(int k, uint64_t g) const { return ptr[k][g + 1] - ptr[k][g]; }
};

// ---- validation of the CSR, totals of the tiled system; the coefficient dictionary and the density maps as they stand before the per-term
// pass (trusted: as they stay)
static inline int plan_validate(SpmvPlan &p, fk_r1cs_dev &r) {
    if (p.copies == 0) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: copies must be at least 1");
    const uint64_t nv = (uint64_t)p.num_input + p.num_aux;
    if (p.num_input == 0) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: num_input must include the constant ONE");
    for (int k = 0; k < 3; k++) {
        if (!p.ptr[k]) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: null row pointer");
        if (p.ptr[k][0] != 0) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: row_ptr[0] must be 0");
        if (p.trusted()) continue;
        for (uint64_t g = 0; g < p.ng; g++) if (p.ptr[k][g + 1] < p.ptr[k][g]) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: row_ptr not monotone");
        const uint64_t nnz = p.ptr[k][p.ng];
        if (nnz && !p.col[k]) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: null column array");   // val[k] == NULL: all coefficients ONE
        if (nnz && p.pre_cidx && !p.pre_cidx[k]) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: null coefficient index array");
        for (uint64_t i = 0; i < nnz; i++) if (p.col[k][i] >= nv) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: variable index %u out of range", p.col[k][i]);
    }
    // totals of the tiled system: ONE is shared, inputs and aux variables are per copy
    const uint64_t t_in = 1 + (uint64_t)p.copies * (p.num_input - 1), t_aux = (uint64_t)p.copies * p.num_aux, t_gates = (uint64_t)p.copies * p.ng;
    if (t_in + t_aux > 0xffffffffull || t_gates + t_in > 0xffffffffull || (p.copies > 1 && p.ng == 0))
        FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: %u copies of this system do not fit 32-bit variable / row indices", p.copies);
    r.num_input = (uint32_t)t_in; r.num_aux = (uint32_t)t_aux; r.num_gates = t_gates;
    r.copies = p.copies; r.base_input = p.num_input; r.base_aux = p.num_aux; r.base_gates = (uint32_t)p.ng;
    const Fr one = Fr::one();
    p.table.assign(1, one);
    p.dict.emplace(std::string((const char *)&one, 32), 0u);
    if (p.pre_cidx) {
        if (!p.pre_table || !p.n_pre_table || p.pre_table[0] != one) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: coefficient table must start with ONE");
        p.table.assign(p.pre_table, p.pre_table + p.n_pre_table);
    }
    p.a_aux.assign(p.num_aux ? p.num_aux : 1, 0); p.b_in.assign(p.num_input, 0); p.b_aux.assign(p.num_aux ? p.num_aux : 1, 0);
    if (p.trusted()) {
        if (p.num_aux) { memcpy(p.a_aux.data(), p.pre_density[0], p.num_aux); memcpy(p.b_aux.data(), p.pre_density[2], p.num_aux); }
        memcpy(p.b_in.data(), p.pre_density[1], p.num_input);
    }
    return FK_OK;
}

// ---- the class lists of one matrix, with block ordering, and where the wave kernel's rows sit in them
static inline void plan_class_list(SpmvPlan &p, fk_r1cs_dev &r, int k, uint64_t bin_min) {
    uint64_t maxlen = 0;
    for (uint64_t g = 0; g < p.ng; g++) if (p.len(k, g) > maxlen) maxlen = p.len(k, g);
    if (!(maxlen >= bin_min && p.ng && p.ng < 0xffffffffull)) return;
    const uint32_t ng = (uint32_t)p.ng, CAP = 1024;            // counting sort by min(length, CAP), descending, stable
    std::vector<uint32_t> cnt(CAP + 2, 0);
    std::vector<uint32_t> &list = r.h_rowlist[k];
    list.resize(ng);
    auto key = [&](uint32_t g) { const uint64_t l = p.len(k, g); return (uint32_t)(l < CAP ? l : CAP); };
    for (uint32_t g = 0; g < ng; g++) cnt[CAP - key(g) + 1]++;
    for (uint32_t i = 0; i <= CAP; i++) cnt[i + 1] += cnt[i];
    for (uint32_t g = 0; g < ng; g++) list[cnt[CAP - key(g)]++] = g;
    // cnt[i] is now the END of key CAP - i
    uint32_t cls_start[SPMV_CLASSES];
    for (int c = 0; c < SPMV_CLASSES; c++) {
        cls_start[c] = c ? cnt[CAP - SPMV_CLS_LO[c - 1]] : 0;
        p.cls_n[k][c] = (SPMV_CLS_LO[c] ? cnt[CAP - SPMV_CLS_LO[c]] : ng) - cls_start[c];
    }
    // A large flat system (a circuit as it comes out of a Parameters file): sorting a class by length over the WHOLE system
    // puts rows from everywhere in the circuit side by side -- every wave then gathers z from all over the witness and
    // streams its matrix entries from all over the CSR.  Sort by length inside blocks of consecutive rows instead: the rows
    // that share a wave still have (nearly) the same length, and what runs at one time reads one window of the circuit
    // (the benchmark's system with every term explicit: evaluation 15.2 -> see profiles/r03_spmv_rollup_probe.log).
    if (p.copies == 1 && SPMV_BLOCK_ROWS && ng >= 16 * SPMV_BLOCK_ROWS) {
        uint32_t pos[SPMV_CLASSES];                            // class c holds the rows of cls_lo[c] <= length < cls_lo[c - 1]
        for (int c = 0; c < SPMV_CLASSES; c++) pos[c] = cls_start[c];
        std::vector<uint32_t> bc(CAP + 2);
        std::vector<uint32_t> tmp(SPMV_BLOCK_ROWS);
        for (uint32_t g0 = 0; g0 < ng; g0 += SPMV_BLOCK_ROWS) {
            const uint32_t g1 = std::min(ng, g0 + SPMV_BLOCK_ROWS);
            std::fill(bc.begin(), bc.end(), 0u);
            for (uint32_t g = g0; g < g1; g++) bc[CAP - key(g) + 1]++;
            for (uint32_t i = 0; i <= CAP; i++) bc[i + 1] += bc[i];
            for (uint32_t g = g0; g < g1; g++) tmp[bc[CAP - key(g)]++] = g;           // the block's rows, longest first (stable)
            for (uint32_t i = 0; i < g1 - g0; i++) {
                const uint32_t l = key(tmp[i]);
                int c = 0;
                while (l < SPMV_CLS_LO[c]) c++;
                list[pos[c]++] = tmp[i];
            }
        }
    }
    r.wave_from[k] = cnt[CAP - SPMV_WAVE_HI]; r.wave_to[k] = cnt[CAP - SPMV_WAVE_LO];             // rows of wave_lo <= length < wave_hi
}

// The class lists of a matrix depend on its row lengths alone: the three are built side by side (a third of a second each for the
// benchmark's 33.5 M rows) before the matrices are uploaded.
static inline int plan_class_lists(SpmvPlan &p, fk_r1cs_dev &r) {
    uint64_t bin_min = 8;          // rows this long make a matrix binned; FK_SPMV_BIN_MIN=0 turns the binned product off (a run-time switch, read per load: the tests run both kernels)
    if (const char *e = getenv("FK_SPMV_BIN_MIN")) { bin_min = strtoull(e, nullptr, 10); if (!bin_min) bin_min = ~0ull; }
    if (p.ng < ((uint64_t)1 << 20)) for (int k = 0; k < 3; k++) plan_class_list(p, r, k, bin_min);
    else if (!side_by_side(3, [&](uint32_t k) { plan_class_list(p, r, (int)k, bin_min); })) FK_SET_ERR(&p, FK_ERR_OOM, "r1cs: out of host memory while ordering the rows");
    // the launch segments of the full lists: one per (binned matrix, class that has rows); a tiled system walks its copies in every segment
    for (uint32_t k = 0; k < 3; k++) {
        if (r.h_rowlist[k].empty()) continue;
        r.bins.mask |= 1u << k;
        uint32_t off = 0;
        for (int c = 0; c < SPMV_CLASSES; c++) {
            if (p.cls_n[k][c]) { FK_TRY(bin_segment(p.err, r.bins, r.bins.nseg, k, SPMV_CLS_LG[c], off, p.cls_n[k][c], (uint64_t)p.cls_n[k][c] * p.copies)); r.bins.nseg++; }
            off += p.cls_n[k][c];
        }
    }
    return FK_OK;
}

// ---- the coefficient coding of matrix k and what it marks in the density maps (one pass over its terms; trusted: none)
static inline int plan_coefficients(SpmvPlan &p, fk_r1cs_dev &r, int k) {
    const uint64_t nnz = p.ptr[k][p.ng];
    r.nnz[k] = nnz * p.copies;
    std::vector<uint32_t> &cidx = p.cidx[k];
    cidx.resize(p.trusted() ? 1 : nnz ? nnz : 1);
    const Fr one = Fr::one();
    Fr last = one; uint32_t last_idx = 0;        // one-entry cache in front of the hash map
    for (uint64_t i = 0; i < nnz && !p.trusted(); i++) {
        uint32_t ci = 0;
        if (p.pre_cidx) {
            ci = p.pre_cidx[k][i];
            if (ci >= p.n_pre_table) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: coefficient index out of range");
        } else if (p.val[k] && memcmp(p.val[k] + 4 * i, &one, 32) != 0) {
            if (memcmp(p.val[k] + 4 * i, &last, 32) == 0) ci = last_idx;
            else {
                std::string key((const char *)(p.val[k] + 4 * i), 32);
                auto it = p.dict.find(key);
                if (it == p.dict.end()) {
                    if (p.table.size() >= 0xffffffffull) FK_SET_ERR(&p, FK_ERR_BAD_ARG, "r1cs: too many distinct coefficients");
                    Fr v; memcpy(&v, p.val[k] + 4 * i, 32);
                    it = p.dict.emplace(key, (uint32_t)p.table.size()).first;
                    p.table.push_back(v);
                }
                ci = it->second; memcpy(&last, p.val[k] + 4 * i, 32); last_idx = ci;
            }
        }
        cidx[i] = ci;
        const uint32_t v = p.col[k][i];
        if (k == 0) { if (v >= p.num_input) p.a_aux[v - p.num_input] = 1; }
        else if (k == 1) { if (v < p.num_input) p.b_in[v] = 1; else p.b_aux[v - p.num_input] = 1; }
    }
    return FK_OK;
}

// ---- row windows for the chunked hand-over of fk_prove_r1cs (r1cs.hpp): explicit systems with block-sorted class lists, every matrix
// binned.  win_need is the loader's: it comes from the columns on the device (spmv.hip: col_window_max_kernel).
static inline void plan_windows(SpmvPlan &p, fk_r1cs_dev &r) {
    if (!(p.copies == 1 && SPMV_WINDOWS >= 2 && SPMV_BLOCK_ROWS && p.ng >= 16ull * SPMV_BLOCK_ROWS && p.ng < 0xffffffffull && r.bins.mask == 7u)) return;
    const uint32_t K = SPMV_WINDOWS;
    for (uint32_t j = 0; j <= K; j++) r.win_row[j] = j == K ? p.ng : (p.ng * j / K) / SPMV_BLOCK_ROWS * SPMV_BLOCK_ROWS;
    for (uint32_t sg = 0; sg < r.bins.nseg; sg++)
        for (uint32_t j = 0; j <= K; j++) r.win_cnt[j][sg] = rows_below(r.h_rowlist[r.bins.mtx[sg]].data() + r.bins.list_off[sg], r.bins.n_rows[sg], r.win_row[j]);
    r.win_k = K;
}

// ---- Alias plan: circuits repeat linear combinations (the Poseidon S-box multiplies a lazily expanded combination by itself: the B row of a
// gate equals its A row, or the A row two gates back) -- 29.6 % of the benchmark transaction's terms sit in such rows.  Which rows repeat is
// a property of the system, not of the witness, and out[dst] = out[src] holds for any z: found once here, see r1cs.hpp.  Gates in row
// order, matrices A, B, C inside a gate; a row of >= dd_min terms is an alias of the EARLIEST row, at most dd_back gates back, that has the
// same columns and coefficient indices (memcmp; the hash only finds candidates) and is not an alias itself.  Rows of a matrix that is not
// binned are sources only.  The bounded look-back makes it one streaming pass with O(dd_back) state, and src row <= dst row.
struct AliasCand { uint64_t key, prev; };       // key = gate * 3 + matrix; prev: the nearest earlier identical row (~0: none)

// pass 1 over the gates [g0, g1), reading dd_back gates into the block before it: the NEAREST earlier identical row of every row that has
// one -- independent of which rows end up as aliases
static inline void alias_scan(const SpmvPlan &p, const uint32_t *const h_cidx[3], uint64_t g0, uint64_t g1, std::vector<AliasCand> &found) {
    const uint64_t R = (uint64_t)SPMV_DD_BACK + 1, NONE = ~0ull;
    std::vector<uint64_t> hs(R * 3), ln(R * 3, 0);              // ring over the last R gates; ln = 0: shorter than dd_min
    for (uint64_t g = g0 > SPMV_DD_BACK ? g0 - SPMV_DD_BACK : 0; g < g1; g++) {
        const size_t slot = (size_t)(g % R) * 3;
        for (int k = 0; k < 3; k++) {
            const uint64_t lo = p.ptr[k][g], len = p.ptr[k][g + 1] - lo;
            ln[slot + k] = 0;
            if (len < SPMV_DD_MIN) continue;
            uint64_t h = len;
            for (uint64_t i = 0; i < len; i++) h = (h ^ (p.col[k][lo + i] | (uint64_t)h_cidx[k][lo + i] << 32)) * 0x9e3779b97f4a7c15ull + (h >> 31);
            hs[slot + k] = h; ln[slot + k] = len;
            if (g < g0) continue;
            auto same = [&](uint64_t g2, int k2) {
                const size_t s2 = (size_t)(g2 % R) * 3 + k2;
                if (ln[s2] != len || hs[s2] != h) return false;
                const uint64_t lo2 = p.ptr[k2][g2];
                return memcmp(p.col[k2] + lo2, p.col[k] + lo, len * 4) == 0 && memcmp(h_cidx[k2] + lo2, h_cidx[k] + lo, len * 4) == 0;
            };
            uint64_t prev = NONE;
            for (int k2 = k - 1; k2 >= 0 && prev == NONE; k2--) if (same(g, k2)) prev = g * 3 + k2;
            for (uint64_t d = 1; d <= SPMV_DD_BACK && d <= g && prev == NONE; d++)
                for (int k2 = 2; k2 >= 0 && prev == NONE; k2--) if (same(g - d, k2)) prev = (g - d) * 3 + k2;
            if (prev != NONE) found.push_back({g * 3 + k, prev});
        }
    }
}

// pass 1 on up to 16 threads over equal blocks of gates from 2^20 gates on; then pass 2 (serial, over the rows that have an identical
// predecessor only): walk the chain of identical rows back through the look-back and take the earliest one that is not an alias
static inline int plan_aliases(SpmvPlan &p, fk_r1cs_dev &r) {
    r.alias_min = SPMV_DD_MIN; r.alias_lookback = SPMV_DD_BACK;
    if (!(p.want_alias && r.bins.mask && p.ng && p.ng < 0xffffffffull)) return FK_OK;
    const uint64_t ng = p.ng, NONE = ~0ull, RS = 3 * ((uint64_t)SPMV_DD_BACK + 1);
    const uint32_t *h_cidx[3];
    for (int k = 0; k < 3; k++) h_cidx[k] = p.pre_cidx ? p.pre_cidx[k] : p.cidx[k].data();
    const uint32_t n_thr = ng >= ((uint64_t)1 << 20) ? std::min(16u, std::max(1u, host_threads())) : 1u;
    try {
        std::vector<std::vector<AliasCand>> found(n_thr);
        if (!side_by_side(n_thr, [&](uint32_t t) { alias_scan(p, h_cidx, ng * t / n_thr, ng * (t + 1) / n_thr, found[t]); })) throw std::bad_alloc();
        struct Seen { uint64_t key, prev; bool alias; };
        std::vector<Seen> ring(RS, Seen{NONE, NONE, false});
        for (auto &blk : found) {
            for (const AliasCand &c : blk) {
                const uint64_t g = c.key / 3; const uint32_t dm = (uint32_t)(c.key % 3);
                Seen &me = ring[c.key % RS];
                me = Seen{c.key, c.prev, false};
                if (!((r.bins.mask >> dm) & 1)) continue;
                uint64_t best = NONE;
                for (uint64_t cur = c.prev; cur != NONE && g - cur / 3 <= SPMV_DD_BACK;) {
                    const Seen &e = ring[cur % RS];
                    const bool known = e.key == cur;         // not known: the row has no identical predecessor in ITS look-back, it is a source
                    if (!known || !e.alias) best = cur;
                    cur = known ? e.prev : NONE;
                }
                if (best == NONE) continue;
                me.alias = true;
                const uint64_t sg = best / 3, sm = best % 3;
                if (p.is_alias[dm].empty()) p.is_alias[dm].assign(ng, 0);
                p.is_alias[dm][g] = 1;
                p.alias.push_back(g | (g - sg) << 32 | (uint64_t)dm << 48 | sm << 50);
                r.alias_terms += p.len(dm, g);
            }
            std::vector<AliasCand>().swap(blk);
        }
    } catch (...) { FK_SET_ERR(&p, FK_ERR_OOM, "r1cs: out of host memory while looking for repeated rows"); }
    return FK_OK;
}

// ---- the dedup set: the class lists without the alias rows -- same class order, same block order, hence the same window prefixes
static inline int plan_dedup(SpmvPlan &p, fk_r1cs_dev &r) {
    if (p.alias.empty()) return FK_OK;
    BinArgs &d = r.bins_dd;
    d.mask = r.bins.mask;
    for (uint32_t s = 0; s < r.bins.nseg; s++) {
        const uint32_t k = r.bins.mtx[s], nr = r.bins.n_rows[s];
        const uint32_t *src = r.h_rowlist[k].data() + r.bins.list_off[s];
        uint32_t off = r.bins.list_off[s], kept = nr;
        if (!p.is_alias[k].empty()) {
            off = (uint32_t)p.dd[k].size();
            for (uint32_t i = 0; i < nr; i++) if (!p.is_alias[k][src[i]]) p.dd[k].push_back(src[i]);
            kept = (uint32_t)p.dd[k].size() - off;
        }
        if (!kept) continue;
        const uint32_t sd = d.nseg++;
        FK_TRY(bin_segment(p.err, d, sd, k, r.bins.lg[s], off, kept, kept));
        const uint32_t *lo = p.is_alias[k].empty() ? src : p.dd[k].data() + off;          // (dd[k] grows no more inside this iteration)
        for (uint32_t j = 0; j <= r.win_k && r.win_k; j++) r.win_cnt_dd[j][sd] = rows_below(lo, kept, r.win_row[j]);
    }
    for (uint32_t j = 0; j <= r.win_k && r.win_k; j++) {
        const uint64_t bound = r.win_row[j];
        r.win_alias[j] = (uint64_t)(std::partition_point(p.alias.begin(), p.alias.end(), [&](uint64_t e) { return (e & 0xffffffffull) < bound; }) - p.alias.begin());
    }
    r.n_alias = p.alias.size();
    return FK_OK;
}

// ---- the wave list of a batch circuit: the rows of wave_lo .. wave_hi - 1 terms of the binned matrices, in circuit order
static inline void plan_wavelist(SpmvPlan &p, fk_r1cs_dev &r) {
    if (!(p.copies > 1 && SPMV_WAVE_COPIES && p.copies >= SPMV_WAVE_COPIES && r.bins.mask && p.ng < ((uint64_t)1 << 30))) return;
    for (uint64_t g = 0; g < p.ng; g++)
        for (uint32_t k = 0; k < 3; k++) {
            const uint64_t l = p.len(k, g);
            if (((r.bins.mask >> k) & 1) && l >= SPMV_WAVE_LO && l < SPMV_WAVE_HI) p.wavelist.push_back(k << 30 | (uint32_t)g);
        }
    if ((uint64_t)((p.copies + 63) / 64) * p.wavelist.size() >= 0xfffffff0ull) p.wavelist.clear();
    r.n_wavelist = (uint32_t)p.wavelist.size();
}

// ---- density maps of the whole batch (every copy repeats the instance's pattern, ONE is shared), their popcounts and the query index lists
// (bellman's order: inputs first, then the aux variables the map selects)
static inline void plan_queries(SpmvPlan &p, fk_r1cs_dev &r) {
    auto rep = [&](std::vector<uint8_t> &f, size_t skip, size_t per) {
        std::vector<uint8_t> o(skip + per * p.copies + (skip + per * p.copies == 0));
        for (size_t i = 0; i < skip; i++) o[i] = f[i];
        for (uint32_t j = 0; j < p.copies; j++) for (size_t i = 0; i < per; i++) o[skip + j * per + i] = f[skip + i];
        f.swap(o);
    };
    if (p.copies > 1) { rep(p.a_aux, 0, p.num_aux); rep(p.b_aux, 0, p.num_aux); rep(p.b_in, 1, p.num_input - 1); }
    r.n_table = p.table.size();
    for (uint32_t j = 0; j < r.num_aux; j++) { r.n_a_aux += p.a_aux[j]; r.n_b_aux += p.b_aux[j]; }
    for (uint32_t i = 0; i < r.num_input; i++) r.n_b_in += p.b_in[i];
    p.idx_a.reserve(r.num_input + r.n_a_aux); p.idx_b.reserve(r.n_b_in + r.n_b_aux);
    for (uint32_t i = 0; i < r.num_input; i++) { p.idx_a.push_back(i); if (p.b_in[i]) p.idx_b.push_back(i); }
    for (uint32_t j = 0; j < r.num_aux; j++) { if (p.a_aux[j]) p.idx_a.push_back(r.num_input + j); if (p.b_aux[j]) p.idx_b.push_back(r.num_input + j); }
}

}  // namespace fk
