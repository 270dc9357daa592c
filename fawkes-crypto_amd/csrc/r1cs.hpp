// The device-resident constraint system (spmv.hip builds and evaluates it; multi.hip keeps one replica per GPU).
#pragma once
#include "common.hpp"
#include <mutex>

namespace fk {
// launch plan of spmv_binned_kernel: up to SPMV_CLASSES length classes for each of the 3 matrices
static constexpr int SPMV_CLASSES = 5, SPMV_SEGS = 3 * SPMV_CLASSES;
struct BinArgs {
    uint32_t nseg = 0, mask = 0;            // mask: bit k = matrix k is binned
    uint32_t first_block[SPMV_SEGS + 1] = {0}, lg[SPMV_SEGS] = {0}, mtx[SPMV_SEGS] = {0}, n_rows[SPMV_SEGS] = {0}, list_off[SPMV_SEGS] = {0};
    const uint32_t *rowlist[3] = {nullptr, nullptr, nullptr};
};
// Cyclic row slices (multi-GPU: rank g of W = 2^log_w evaluates only the rows t = g (mod W), the slice the distributed
// quotient starts from).  The length-class lists are kept a second time per log_w with every class grouped by row mod W
// (inside a group still longest first), so that a rank's rows of a class are one contiguous run per copy; which residue a
// copy needs depends on the copy (row t = copy * base_gates + row), with period P = W / gcd(base_gates, W) copies.
struct SliceLists {
    DevArr<uint32_t> d_list[3];                           // per matrix, same length and class boundaries as rowlist
    uint32_t cnt[SPMV_SEGS][8] = {{0}}, offs[SPMV_SEGS][8] = {{0}};       // per segment: rows of each residue / their first position in the class
    bool built = false;
};
struct SliceArgs {
    uint32_t log_w = 0, rank = 0, P = 1;
    uint32_t rho[8] = {0};                 // residue copy q*P + p needs
    uint32_t T[SPMV_SEGS] = {0};           // groups of one period of copies, per segment
    uint32_t cnt[SPMV_SEGS][8] = {{0}}, offs[SPMV_SEGS][8] = {{0}};
};
}  // namespace fk

// Every device array is a DevArr: deleting the object frees them all (fk_r1cs_free), as does any early return of the loader (spmv_plan.hpp fills the plain fields).
struct fk_r1cs_dev {
    uint32_t num_input = 0, num_aux = 0;
    uint64_t num_gates = 0;
    fk::DevArr<uint64_t> ptr[3];
    fk::DevArr<uint32_t> col[3], cidx[3];
    fk::DevArr<fk::Fr> table;
    uint64_t n_table = 0, nnz[3] = {0, 0, 0};
    fk::DevArr<uint8_t> d_a_aux, d_b_in, d_b_aux;
    uint64_t n_a_aux = 0, n_b_in = 0, n_b_aux = 0;   // popcounts
    fk::DevArr<uint32_t> d_idx_a, d_idx_b;           // variables of the A / B query in query order
    fk::QueryIdx qidx;
    // tiled system (fk_r1cs_load_tiled): the CSR above is ONE instance (base_gates rows, base_input / base_aux variables)
    // and stands for `copies` of it; num_input / num_aux / num_gates / nnz are the totals
    uint32_t copies = 1, base_input = 0, base_aux = 0, base_gates = 0;
    // matrices with long rows: the (instance's) rows in classes by length, sorted by length inside a class (see spmv_binned_kernel)
    fk::DevArr<uint32_t> rowlist[3];
    fk::BinArgs bins;
    // batch circuits of >= 64 copies: the rows of middling length that spmv_tiled_wave_kernel takes (matrix << 30 | row, circuit
    // order) and where they sit in rowlist (sorted by length: [wave_from, wave_to) of each matrix)
    fk::DevArr<uint32_t> d_wavelist;
    uint32_t n_wavelist = 0, wave_from[3] = {0, 0, 0}, wave_to[3] = {0, 0, 0};
    // Row windows (explicit systems whose class lists are block-sorted, all three matrices binned): the gate rows cut into win_k runs of
    // consecutive rows.  win_cnt[j][s]: entries of launch segment s whose row lies below win_row[j] (a PREFIX of the segment's list: the
    // lists are ordered by blocks of consecutive rows); win_need[j]: how many leading elements of z the rows below win_row[j + 1] read.
    // fk_prove_r1cs uploads z in those pieces and evaluates window j as soon as piece j has landed (spmv.hip: prove_r1cs_chunked).
    static constexpr uint32_t WIN_MAX = 16;
    uint32_t win_k = 0;
    uint64_t win_row[WIN_MAX + 1] = {0}, win_need[WIN_MAX] = {0};
    uint32_t win_cnt[WIN_MAX + 1][fk::SPMV_SEGS] = {{0}};
    // Repeated linear combinations (explicit systems, found once at load: spmv_plan.hpp, alias plan).  Row (dm, drow) of a binned matrix whose
    // columns and coefficient indices are byte-identical to those of an earlier, non-alias row (sm, srow) at most alias_lookback gates
    // back is an ALIAS: the unsliced evaluation leaves it out of the class lists (the dedup set: rowlist_dd / bins_dd / win_cnt_dd, the
    // same class and block order as rowlist / bins / win_cnt) and spmv_alias_kernel copies out[sm][srow] to out[dm][drow] behind it.
    // d_alias: drow | (drow - srow) << 32 | dm << 48 | sm << 50, sorted by (drow, dm); win_alias[j]: aliases whose drow < win_row[j].
    // The sliced and the tiled evaluations and h_rowlist keep the full lists.
    fk::DevArr<uint64_t> d_alias;
    uint64_t n_alias = 0, alias_terms = 0;
    uint32_t alias_min = 0, alias_lookback = 0;
    fk::DevArr<uint32_t> rowlist_dd[3];              // only for the matrices that have aliases; bins_dd points at rowlist for the others
    fk::BinArgs bins_dd;
    uint32_t win_cnt_dd[WIN_MAX + 1][fk::SPMV_SEGS] = {{0}};
    uint64_t win_alias[WIN_MAX + 1] = {0};
    // host copies of the class lists and the per-log_w residue-grouped variants, built on first use (fk_r1cs_eval_slice_dev)
    std::vector<uint32_t> h_rowlist[3];
    mutable fk::SliceLists slices[4];
    mutable std::mutex slice_mu;
};

namespace fk {
// A resident system's queries as a run of the prover takes them (common.hpp: ProveRun): its index lists, no per-proof compaction.
static inline WitnessQueries r1cs_queries(const fk_r1cs_dev *r) { return {r->d_a_aux, r->d_b_in, r->d_b_aux, &r->qidx}; }
// The one check that a system belongs to a key.  rows (may be null: only the witness multiplications follow, no transform): the rows
// a, b, c get -- the gates and one row per input -- which must fill more than half of the key's domain and no more than all of it.
static inline int r1cs_fits_key(fk_ctx *ctx, const fk_r1cs_dev *r, const fk_key *key, uint64_t *rows) {
    if (r->num_input != key->num_input || r->num_aux != key->num_aux) FK_SET_ERR(ctx, FK_ERR_KEY_MISMATCH, "prove: constraint system and key disagree on the variable counts");
    if (!rows) return FK_OK;
    *rows = r->num_gates + r->num_input;
    if (*rows > key->m || (key->m > 1 && *rows <= key->m / 2)) FK_SET_ERR(ctx, FK_ERR_KEY_MISMATCH, "prove: %llu rows do not match key domain %llu",
                                                                       (unsigned long long)*rows, (unsigned long long)key->m);
    return FK_OK;
}
// The key refusals that the per-proof and the batch prover share (the tests compare codes and texts).
// A resident system's A / B query sizes against the key's arrays:
static inline int queries_fit_key(fk_ctx *ctx, const QueryIdx *qi, const fk_key *key) {
    if (qi->n_b != key->n_b) FK_SET_ERR(ctx, FK_ERR_KEY_MISMATCH, "prove: b query needs %llu points, key holds %llu", (unsigned long long)qi->n_b, (unsigned long long)key->n_b);
    if (qi->n_a != key->n_a) FK_SET_ERR(ctx, FK_ERR_KEY_MISMATCH, "prove: a query needs %llu points, key holds %llu", (unsigned long long)qi->n_a, (unsigned long long)key->n_a);
    return FK_OK;
}
// the key's l and h arrays against its own domain and variable counts (the batch prover reads l by variable and h by row)
static inline int key_arrays_whole(fk_ctx *ctx, const fk_key *key) {
    if (key->n_l != key->num_aux || key->n_h + 1 != key->m) FK_SET_ERR(ctx, FK_ERR_KEY_MISMATCH, "prove: key arrays do not match its domain and variable counts");
    return FK_OK;
}
// bellman's UnexpectedIdentity: no proof under a key whose delta is the point at infinity
static inline int key_delta_ok(fk_ctx *ctx, const fk_key *key) {
    if (key->delta_g1.is_inf() || key->delta_g2.is_inf()) FK_SET_ERR(ctx, FK_ERR_UNEXPECTED_IDENTITY, "delta is the identity");
    return FK_OK;
}
// spmv.hip
int r1cs_load_coded(fk_ctx *ctx, uint32_t num_input, uint32_t num_aux, uint64_t num_gates, const uint64_t *const ptr[3], const uint32_t *const col[3],
                    const uint32_t *const cidx[3], const Fr *table, uint64_t n_table, fk_r1cs_dev **out, const uint8_t *const density[3] = nullptr);
int r1cs_eval_impl(fk_ctx *ctx, const fk_r1cs_dev *r, const void *d_z, void *d_a, void *d_b, void *d_c, bool sliced, uint32_t rank, uint32_t log_w, uint64_t n_out, int window);
int prove_r1cs_dev_impl(fk_ctx *ctx, const fk_key *key, const fk_r1cs_dev *r, const void *d_z, const uint64_t rr[4], const uint64_t ss[4],
                        uint8_t out_proof[FK_PROOF_BYTES], fk_timings *tm, const std::function<int()> *after_eval, const std::function<int()> *before_block);
}  // namespace fk
