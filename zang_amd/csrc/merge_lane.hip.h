// merge_lane.hip.h -- the per-lane walk of the merge stage (span_merge.hip), written once as a __host__ __device__ function, the
// row stores included, so that the same text runs in a CPU harness (tests/cpp/merge_lane_host.cpp).  One call of merge_lane is the
// loop of examples/example_two.zig:93-151 for one player without its voice: two sources' sub-span rows, each the results of one
// Trigger, cut at every end of either into the rows of one table.  The walk keeps no state: the Triggers live where the sources'
// tables were made.  Semantics and what is defined where the reference is not: zang_hip.h.
#pragma once
#include "span_stage.hip.h"
#define MERGE_HD STAGE_HD

constexpr uint32_t kMergeMaxFields = 4;     // per source
enum { MERGE_NOTE_ON = 0, MERGE_NIC_A, MERGE_NIC_B, kMergeOwnFields };   // the stage's own fields, after A's and B's

// one source: a [span][player] table and its field arrays, words of either kind
struct MergeSrc {
    uint32_t max_spans, n_fields;
    const uint32_t *count, *end;            // `start` is never read (:99, :105-108: a row begins where the last one ended)
    const uint8_t *nic;
    const uint32_t *on;                     // the note-on field's array (one of field[])
    const uint32_t *field[kMergeMaxFields];
};
using MergeOut = StageRows;                 // the stage's table: n_a + n_b + kMergeOwnFields fields
// player p of n: rows [0, count) of the output, count <= max_spans; -> the rows that did not fit
MERGE_HD uint32_t merge_lane(const MergeSrc &A, const MergeSrc &B, const StageRows &o, size_t n, size_t p, uint32_t out_len, uint32_t max_spans) {
    const uint32_t ca = A.count[p], cb = B.count[p];
    const uint32_t cnt_a = ca < A.max_spans ? ca : A.max_spans, cnt_b = cb < B.max_spans ? cb : B.max_spans;
    uint32_t pos = 0, ia = 0, ib = 0;                                 // :99; trig.next once per source (:96-97)
    StageWriter out{o, n, p, max_spans, 0, 0};
    while (pos < out_len && ia < cnt_a && ib < cnt_b) {               // :101, :103-104; a source without a row: the break of :150
        const size_t ra = (size_t)ia * n + p, rb = (size_t)ib * n + p;
        const uint32_t ea = A.end[ra], eb = B.end[rb];
        const uint32_t e = ea < eb ? ea : eb;                         // :107
        if (e <= pos || e > out_len) break;                           // no Trigger makes such a row: it ends the list
        out.row(pos, e, [&](size_t idx) {
            const uint32_t on_a = A.on[ra] != 0 ? 1u : 0u, on_b = B.on[rb] != 0 ? 1u : 0u;
            // result0 / result1 stay the same objects until their trig.next runs: a source's note_id_changed sticks
            const uint32_t nic_a = A.nic[ra] != 0 ? 1u : 0u, nic_b = B.nic[rb] != 0 ? 1u : 0u;
            o.changed[idx] = (uint8_t)((nic_a & on_a & (nic_b ^ 1u)) | (nic_b & on_b & (nic_a ^ 1u)));   // :127-129
            uint32_t *w = o.words + idx;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (uint32_t i = 0; i < kMergeMaxFields; i++)
                if (i < A.n_fields) { *w = A.field[i][ra]; w += o.plane; }
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (uint32_t i = 0; i < kMergeMaxFields; i++)
                if (i < B.n_fields) { *w = B.field[i][rb]; w += o.plane; }
            w[(size_t)MERGE_NOTE_ON * o.plane] = on_a | on_b;         // :136
            w[(size_t)MERGE_NIC_A * o.plane] = nic_a;
            w[(size_t)MERGE_NIC_B * o.plane] = nic_b;
        });
        if (ea == e) ia++;                                            // :139-144: both advance on a tie
        if (eb == e) ib++;
        pos = e;                                                      // :145
    }
    o.count[p] = out.k;
    return out.dropped;
}
