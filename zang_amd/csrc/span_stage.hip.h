// span_stage.hip.h -- what the stages that FILL a [span][player] sub-span table share (sched_bank.hip, arp.hip, subsong.hip,
// span_merge.hip); the sibling of span_voice.hip.h, which serves the voices that read such a table.  Two parts:
//   the table as a lane sees it and the writer that takes one player's rows into it, as plain C++ (the stand-alone harnesses of
//   tests/cpp include it, so the row store they run under ASan is the one the kernels run);
//   the host side (hipcc only): the table's allocations with alloc / free / reserve, the views the ABI hands out, the overflow
//   count, and the check of a table that comes IN.
// A stage's translation unit is then its kernel, its handle (a zh_stage plus what is its own) and the extern "C" wrappers.
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STAGE_HD __host__ __device__ inline
#else
#define STAGE_HD inline
#endif

// A stage's table: row k of player p of n at k * n + p; field f of that row at words[f * plane + k * n + p], plane = capacity
// rows x n (the capacity, not the max_spans of one schedule).
struct StageRows {
    uint32_t *count, *start, *end;
    uint8_t *changed;
    uint32_t *words;
    size_t plane;
    // a row of two fields (the arp and subsong lanes'): 0 = freq as its bits, 1 = note_on
    STAGE_HD void freq_on(size_t idx, uint32_t freq_bits, uint32_t note_on, uint32_t nic) const {
        words[idx] = freq_bits; words[plane + idx] = note_on; changed[idx] = (uint8_t)nic;
    }
};

// One player's rows, in order: the list stops at max_spans, what does not fit is counted.  {t, n, p, max_spans, 0, 0}; afterwards
// t.count[p] = k is the caller's, and `dropped` goes to the stage's overflow count.  Rows: StageRows (StageWriter), or another
// holder of start / end arrays with a freq_on (subsong_lane.hip.h SubsongRowsP).
template <class Rows> struct StageWriterT {
    Rows t;
    size_t n, p;
    uint32_t max_spans, k, dropped;
    // the next row [s0, s1): fill(idx) writes what else it has (fields at t.words + idx, `changed` at t.changed + idx) -- or dropped.
    // (fill runs INSIDE the one branch: with the index handed back for the caller to test, every kernel got a second one.)
    template <class Fill> STAGE_HD void row(uint32_t s0, uint32_t s1, Fill &&fill) {
        if (k >= max_spans) { dropped++; return; }
        const size_t idx = (size_t)k * n + p;
        t.start[idx] = s0; t.end[idx] = s1;
        fill(idx);
        k++;
    }
    // the `emit` of the arp and subsong lanes
    STAGE_HD void operator()(uint32_t s0, uint32_t s1, uint32_t freq_bits, uint32_t note_on, uint32_t changed) {
        row(s0, s1, [&](size_t idx) { t.freq_on(idx, freq_bits, note_on, changed); });
    }
};
using StageWriter = StageWriterT<StageRows>;

#if defined(__HIPCC__)
#include "common.hip.h"

// ---- the host side -----------------------------------------------------------------------------------------------------
// n: players (a bank's voices); count [n] and overflow [1] live as long as the table, the rest is reallocated by reserve
struct StageTable {
    uint32_t n, fields, rows;
    uint32_t *count, *overflow;
    uint32_t *start, *end, *words;       // [rows][n]; words [fields][rows][n]
    uint8_t *changed;
};
// the base of the stages' opaque handles (zh_voice_bank, zh_arp, zh_subsong, zh_span_merge)
struct zh_stage {
    zh_ctx *ctx;
    StageTable tab;
};

static void stage_free_rows(StageTable &t) {
    (void)hipFree(t.start); (void)hipFree(t.end); (void)hipFree(t.words); (void)hipFree(t.changed);
    t.start = t.end = t.words = nullptr; t.changed = nullptr; t.rows = 0;
}
static void stage_free(StageTable &t) {
    stage_free_rows(t);
    (void)hipFree(t.count); (void)hipFree(t.overflow);
    t.count = t.overflow = nullptr;
}
static int stage_alloc_rows(StageTable &t, uint32_t rows) {
    const size_t cells = (size_t)rows * t.n;
    int rc = dev_alloc(&t.start, cells);
    if (!rc) rc = dev_alloc(&t.end, cells);
    if (!rc) rc = dev_alloc(&t.words, cells * t.fields);
    if (!rc) rc = dev_alloc(&t.changed, cells);
    if (rc) { stage_free_rows(t); (void)hipGetLastError(); return rc; }
    t.rows = rows;
    return ZH_OK;
}
// a zeroed handle's table: `rows` rows, no overflow, every list empty
static int stage_create(zh_stage *s, uint32_t n, uint32_t fields, uint32_t rows) {
    StageTable &t = s->tab;
    t.n = n; t.fields = fields;
    int rc = dev_alloc(&t.count, (size_t)n);
    if (!rc) rc = dev_alloc(&t.overflow, 1);
    if (!rc) rc = stage_alloc_rows(t, rows);
    if (!rc) rc = (int)hipMemsetAsync(t.overflow, 0, 4, s->ctx->stream);
    if (!rc && n) rc = (int)hipMemsetAsync(t.count, 0, (size_t)n * 4, s->ctx->stream);
    return rc;
}
// a create that failed with rc: what it enqueued may be in flight; free_all(h) frees the table and what is the stage's own
template <class H> static int stage_create_failed(H *h, void (*free_all)(H *), int rc) {
    (void)hipStreamSynchronize(h->ctx->stream);
    free_all(h);
    delete h;
    (void)hipGetLastError();
    return rc;
}
template <class H> static int stage_destroy(H *h, void (*free_all)(H *)) {
    if (!h) return ZH_ERR_INVALID;
    if (!h->ctx->capturing) (void)hipStreamSynchronize(h->ctx->stream);
    free_all(h);
    delete h;
    return ZH_OK;
}
// zh_*_reserve: the same capacity changes nothing; any other invalidates every view (the stream is idle before the rows go)
static int stage_reserve(zh_stage *s, uint32_t max_rows) {
    if (!s || max_rows == 0) return ZH_ERR_INVALID;
    if (s->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    if (max_rows == s->tab.rows) return ZH_OK;
    ZH_TRY(hipStreamSynchronize(s->ctx->stream));
    stage_free_rows(s->tab);
    return stage_alloc_rows(s->tab, max_rows);
}
// what a schedule and a view may ask for: 1 .. capacity
static bool stage_spans_ok(const zh_stage *s, uint32_t max_spans) { return s && max_spans != 0 && max_spans <= s->tab.rows; }
static StageRows stage_rows(const zh_stage *s) {
    const StageTable &t = s->tab;
    return StageRows{t.count, t.start, t.end, t.changed, t.words, (size_t)t.rows * t.n};
}
static int stage_script_table(const zh_stage *s, uint32_t max_spans, zh_script_span_table *out) {
    if (!out || !stage_spans_ok(s, max_spans)) return ZH_ERR_INVALID;
    *out = zh_script_span_table{max_spans, 0, s->tab.count, s->tab.start, s->tab.end, s->tab.changed};
    return ZH_OK;
}
// field `field` as the array of its kind: 'f', 'u', or 0 = a record word, either view
static int stage_span_param(const zh_stage *s, uint32_t field, char kind, zh_script_span_param *out) {
    if (!s || !out || field >= s->tab.fields) return ZH_ERR_INVALID;
    const uint32_t *w = s->tab.words + (size_t)field * s->tab.rows * s->tab.n;
    *out = zh_script_span_param{kind == 'u' ? nullptr : (const float *)w, kind == 'f' ? nullptr : w};
    return ZH_OK;
}
static int stage_overflows(zh_stage *s, uint64_t *out) {
    if (!s || !out) return ZH_ERR_INVALID;
    uint32_t w = 0;
    int rc = zh_download(s->ctx, &w, s->tab.overflow, 4);
    *out = w;
    return rc;
}
// a table that comes in: a whole one (its start too, though no stage reads it); `nic`: note_id_changed is read as well
static bool stage_input_ok(const zh_script_span_table *t, bool nic) {
    return t && t->max_spans != 0 && t->count && t->start && t->end && (!nic || t->note_id_changed);
}
#endif   // __HIPCC__
