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

/* A adopts L's bucket sort (csrc/msm.hip: key_a_pad) where both slices of the key are whole, the domain is at most 2^25 and a resident
 * constraint system gives the A query: the key then keeps A's aux bases a second time, laid out in L's index space (infinity where a variable
 * takes no part in A) with levels of their own, beside a's array and levels, which stay as they are.  One such array per A query, at most
 * two per key, each built by the first proof that meets its query, under a lock of the key; a proof never changes or frees one (contexts in
 * other threads may be reading it), fk_key_drop_levels / fk_key_derive_levels / fk_key_free release them.  FK_PROVE_SHARE_AL_SORT=0 keeps A's
 * own sort.  out[6] = arrays in place, points of one, levels it holds, queries refused (the forms of a and l differ, or no room: A keeps its
 * own sort), queries seen, bytes of HBM the arrays and their levels occupy. */
int fk_key_a_pad_info(const fk_key *key, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
