/* Inspection entry points of libfawkes_hip.so that only the tests call.  They are exported by the library and deliberately kept out of
 * fawkes_hip.h and its mirrors (the Rust shim, INTEGRATION.md, the ctypes table): the public ABI those describe is what an integrator
 * calls, and tests/test_ffi_mirror.py pins its extent.  A test declares the argument types itself. */
#ifndef FAWKES_HIP_INSPECT_H
#define FAWKES_HIP_INSPECT_H
#include "fawkes_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The alias plan of a resident constraint system (csrc/r1cs.hpp): rows whose linear combination repeats an earlier row's exactly and are
 * therefore copied instead of evaluated.  out[4] = aliases, matrix terms they stand for, minimum row length in force (FK_SPMV_DEDUP_MIN),
 * look-back in gates in force (FK_SPMV_DEDUP_LOOKBACK).  No aliases: tiled system, nothing binned, FK_SPMV_DEDUP=0, or no repeats. */
int fk_r1cs_alias_info(const fk_r1cs_dev *r1cs, uint64_t out[4]);
/* the table, sorted by (dst row, dst matrix); matrices 0 = A, 1 = B, 2 = C; cap: elements each array holds (>= out[0] above) */
int fk_r1cs_aliases(const fk_r1cs_dev *r1cs, uint64_t cap, uint32_t *dst_mtx, uint32_t *dst_row, uint32_t *src_mtx, uint32_t *src_row);

/* The plan the loader of a resident constraint system makes, on the host alone: no context, no GPU.  It runs the loader's own stages
 * (csrc/spmv_plan.hpp) over `cs` standing for `copies` of itself and reports what they decide.  a_cidx / b_cidx / c_cidx, table, n_table: as
 * fk_r1cs_load_coded takes them, or all NULL / 0 for the coefficients of `cs` (its *_val; NULL there: every coefficient ONE).
 * The caller allocates the arrays of `out` (any may be NULL: not wanted): list / list_dd num_gates elements each, the four alias arrays
 * 3 * num_gates, idx_a / idx_b as many as the `copies` systems have variables.  A refusal returns the loader's code; fk_last_error(NULL)
 * has its text.  Row windows: win_need is not reported, it is read off the columns on the device. */
#define FK_PLAN_SEGS 15
#define FK_PLAN_WIN_MAX 16
typedef struct {
    uint32_t nseg, mask;                          /* mask: bit k = matrix k has class lists */
    uint32_t mtx[FK_PLAN_SEGS], lg[FK_PLAN_SEGS], rows[FK_PLAN_SEGS], list_off[FK_PLAN_SEGS], first_block[FK_PLAN_SEGS + 1];
} fk_r1cs_plan_segs;
typedef struct {
    uint32_t *list[3];                            /* in: the class lists, per matrix (written where the matrix is binned) */
    uint32_t *list_dd[3];                         /* in: the dedup lists (written where own_dd[k]; n_dd[k] entries) */
    uint32_t *alias_dst_mtx, *alias_dst_row, *alias_src_mtx, *alias_src_row;     /* in: the alias table as fk_r1cs_aliases gives it */
    uint32_t *idx_a, *idx_b;                      /* in: the A / B query index lists */
    fk_r1cs_plan_segs segs, segs_dd;              /* the launch segments of the full lists and of the dedup lists (n_alias > 0) */
    uint32_t own_dd[3], n_dd[3];                  /* matrix k has a dedup list of its own (else its segments of segs_dd point into list[k]) */
    uint32_t wave_from[3], wave_to[3];            /* list[k][wave_from .. wave_to): the rows the tiled wave kernel takes */
    uint32_t win_k;                               /* row windows (0: none) */
    uint64_t win_row[FK_PLAN_WIN_MAX + 1], win_alias[FK_PLAN_WIN_MAX + 1];
    uint32_t win_cnt[FK_PLAN_WIN_MAX + 1][FK_PLAN_SEGS], win_cnt_dd[FK_PLAN_WIN_MAX + 1][FK_PLAN_SEGS];
    uint64_t n_alias, alias_terms, alias_min, alias_lookback;
    uint64_t n_idx_a, n_idx_b;
} fk_r1cs_plan_info;
int fk_r1cs_plan_host(const fk_r1cs *cs, uint32_t copies, const uint32_t *a_cidx, const uint32_t *b_cidx, const uint32_t *c_cidx, const uint64_t *table,
                      uint64_t n_table, fk_r1cs_plan_info *out);

/* A adopts L's bucket sort (csrc/msm.hip: key_a_pad) where both slices of the key are whole, the domain is at most 2^25 and a resident
 * constraint system gives the A query: the key then keeps A's aux bases a second time, laid out in L's index space (infinity where a variable
 * takes no part in A) with levels of their own, beside a's array and levels, which stay as they are.  One such array per A query, at most
 * two per key, each built by the first proof that meets its query, under a lock of the key; a proof never changes or frees one (contexts in
 * other threads may be reading it), fk_key_drop_levels / fk_key_derive_levels / fk_key_free release them.  FK_PROVE_SHARE_AL_SORT=0 keeps A's
 * own sort.  out[6] = arrays in place, points of one, levels it holds, queries refused (the forms of a and l differ, or no room: A keeps its
 * own sort), queries seen, bytes of HBM the arrays and their levels occupy. */
int fk_key_a_pad_info(const fk_key *key, uint64_t out[6]);

/* The back of one multiplication, stage by stage (csrc/msm.hip; tests/test_gpu_msm_back.py): one whole multiplication over n device-resident
 * bases (G1Affine, g2 != 0: G2Affine) and Montgomery scalars under the context's window bits, queued by the product's own host code
 * (msm_reserve, queue_sort, queue_size_order, queue_accumulate, queue_tail, msm_end) on the next lane in turn, with the lane synchronised
 * between the pieces so that what every kernel left can be copied out.  merged != 0: the one-bucket-set form; the levels of the bases are
 * built here by the loop a key's are built by, and freed again.  The caller allocates the arrays of `out`; any may be NULL (not wanted).
 * With p = fk_msm_plan(n, window bits, merged), WR = merged ? 1 : p.W bucket sets of p.B buckets, points as the device holds them (Xyzz:
 * x, y, zz, zzz Montgomery limb images, 4 x 32 bytes in G1, 4 x 64 in G2; zz = 0: infinity):
 *   sorted p.W * n, starts / totals p.W * p.B, perm p.W * p.B (merged: perm[p.B], then the merged lengths mt[p.B]), dyn, tasks (2 words
 *   each, at most tasks_cap), obs (3 words each, at most obs_cap): as fk_msm_front_dump gives them;
 *   buckets_acc: the WR * p.B buckets behind the accumulation; buckets: the same behind msm_overflow_fold_kernel -- both only when
 *   WR * p.B <= buckets_cap; partials: dyn.n_tasks points (at most partials_cap); winparts: WR * p.nblk points; folded: WR points;
 *   result: the point msm_end returns; levels (merged): (p.W - 1) * n affine points, level w at (w - 1) * n.
 * Refused while a proof holds the lanes; the lane forgets the sort, no tail record stays active.  n = 0: FK_OK, nothing written. */
typedef struct {
    uint32_t *sorted, *starts, *totals, *perm;
    fk_msm_dyn_info *dyn;
    uint32_t *tasks; size_t tasks_cap;
    uint32_t *obs; size_t obs_cap;
    void *buckets_acc, *buckets; size_t buckets_cap;
    void *partials; size_t partials_cap;
    void *winparts, *folded, *result, *levels;
} fk_msm_back_out;
int fk_msm_back_dump(fk_ctx *ctx, int g2, const void *d_bases, const void *d_scalars, size_t n, int merged, const fk_msm_back_out *out);

#ifdef __cplusplus
}
#endif
#endif
