// What batch_prove.hip and batch_check.hip share: where a variable of a proof lives, and the hand-over of a group's evaluated rows
// from the prover's loop to the per-proof check.
#pragma once
#include "common.hpp"
#include "../../include/fawkes_hip_batch_check.h"

namespace fk {

// ------------------------------------------------------------------------------------------ where a variable lives
// ONE function of (layout, proof, variable): every stage that reads z goes through it, the host reference of the check included.
struct ZView {
    const Fr *z;
    int layout;
    uint32_t num_input, num_aux;     // FK_BATCH_Z_TILED
    uint32_t count, p0;              // proofs of the whole call (the tiled order depends on it); first proof of this group
    uint64_t row;                    // FK_BATCH_Z_ROWS: elements per row
};
static FK_HD uint64_t zaddr(const ZView &v, uint32_t proof, uint32_t var) {
    const uint64_t p = (uint64_t)v.p0 + proof;
    if (v.layout == FK_BATCH_Z_ROWS) return p * v.row + var;
    if (var == 0) return 0;
    if (var < v.num_input) return 1 + p * (v.num_input - 1) + (var - 1);
    return 1 + (uint64_t)v.count * (v.num_input - 1) + p * v.num_aux + (var - v.num_input);
}

// ------------------------------------------------------------------------------------------ the per-proof check (batch_check.hip)
// Where the verdicts of a call go: the caller's device arrays (either may be null) and host reports, all indexed by the proof's place
// in the whole call.
struct BatchCheckSink {
    unsigned long long *d_bitmap;    // count x ceil(gates / 64) words
    uint8_t *d_proof_bad;            // count bytes
    fk_check_report *reports;        // count records, host
};
// the records of a group of at most `group` proofs in ctx->bt_check (grow-only: before anything of the call is queued)
int batch_check_reserve(fk_ctx *ctx, uint32_t group);
// Queues FK_BATCH_CHECK_LAUNCHES launches behind the evaluation of the g proofs [zv.p0, zv.p0 + g): a, b, c are the group's rows, proof-major
// with stride m, and must stay as they are until these launches have run (stream order does that for the quotient behind them).
int batch_check_queue(fk_ctx *ctx, const BatchCheckSink &sink, const ZView &zv, const Fr *a, const Fr *b, const Fr *c, uint64_t gates, uint64_t m, uint32_t g);
// queues the download of the group's records into sink.reports[p0 ..]; they are there once the stream has been waited for
int batch_check_download(fk_ctx *ctx, const BatchCheckSink &sink, uint32_t p0, uint32_t g);

}  // namespace fk
