// span_merge.hip -- the merge stage: the loop of examples/example_two.zig:93-151 without its voice, for n players on the device.
// k_span_merge, one lane per player, reads two [span][player] sub-span tables with their field arrays (two live voice banks of
// polyphony 1, say) and writes the stage's own table, which the span paints read in place: one voice driven by two impulse
// streams.  The stage keeps no state between buffers.  The per-lane walk is merge_lane.hip.h; semantics and what is defined where
// the reference is not: zang_hip.h.
#include "common.hip.h"
#include "merge_lane.hip.h"
#include <new>
#include <string.h>

static_assert((int)ZH_SPAN_MERGE_MAX_FIELDS == (int)kMergeMaxFields && (int)ZH_SPAN_MERGE_OWN_FIELDS == (int)kMergeOwnFields &&
              (int)ZH_SPAN_MERGE_NOTE_ON == (int)MERGE_NOTE_ON && (int)ZH_SPAN_MERGE_NIC_A == (int)MERGE_NIC_A &&
              (int)ZH_SPAN_MERGE_NIC_B == (int)MERGE_NIC_B, "the lane's fields are the header's");

namespace {
constexpr uint32_t kMergeBlock = 64;
constexpr uint32_t kMergeDefaultRows = 67;                            // two 34-row tables: 34 + 34 - 1 cuts

struct MergeArgs {
    uint32_t n, out_len, max_spans;
    MergeSrc a, b;
    MergeOut out;
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kMergeBlock) k_span_merge(const MergeArgs g) {
    const uint32_t p = blockIdx.x * kMergeBlock + threadIdx.x;
    if (p >= g.n) return;
    const uint32_t dropped = merge_lane(g.a, g.b, g.out, g.n, p, g.out_len, g.max_spans);
    if (dropped) atomicAdd(g.overflow, dropped);
}
}  // namespace

struct zh_span_merge {
    zh_ctx *ctx;
    uint32_t n, rows;
    zh_span_merge_source a, b;
    uint32_t *count, *start, *end, *words;                            // words: [a.n_fields + b.n_fields + 3][rows][n]
    uint8_t *changed;
    uint32_t *overflow;
};

namespace {
uint32_t merge_fields(const zh_span_merge *m) { return m->a.n_fields + m->b.n_fields + kMergeOwnFields; }
void merge_free_tables(zh_span_merge *m) {
    (void)hipFree(m->start); (void)hipFree(m->end); (void)hipFree(m->words); (void)hipFree(m->changed);
    m->start = m->end = m->words = nullptr; m->changed = nullptr; m->rows = 0;
}
void merge_free(zh_span_merge *m) {
    merge_free_tables(m);
    (void)hipFree(m->count); (void)hipFree(m->overflow);
}
int merge_alloc_tables(zh_span_merge *m, uint32_t rows) {
    const size_t cells = (size_t)rows * m->n;
    int rc = dev_alloc(&m->start, cells);
    if (!rc) rc = dev_alloc(&m->end, cells);
    if (!rc) rc = dev_alloc(&m->words, cells * merge_fields(m));
    if (!rc) rc = dev_alloc(&m->changed, cells);
    if (rc) { merge_free_tables(m); (void)hipGetLastError(); return rc; }
    m->rows = rows;
    return ZH_OK;
}
bool merge_source_ok(const zh_span_merge_source *s) {
    if (!s || s->n_fields == 0 || s->n_fields > kMergeMaxFields || s->on_field >= s->n_fields) return false;
    for (uint32_t i = 0; i < s->n_fields; i++)
        if (s->kinds[i] != 'f' && s->kinds[i] != 'u') return false;
    return s->kinds[s->on_field] == 'u';
}
// a source's table and field arrays -> the lane's view; false: something the schedule refuses
bool merge_src(const zh_span_merge_source &d, const zh_script_span_table *t, const zh_script_span_param *f, MergeSrc &s) {
    if (!t || !f || t->max_spans == 0 || !t->count || !t->start || !t->end || !t->note_id_changed) return false;   // start: a whole table, though never read
    s = MergeSrc{t->max_spans, d.n_fields, t->count, t->end, t->note_id_changed, nullptr, {nullptr, nullptr, nullptr, nullptr}};
    for (uint32_t i = 0; i < d.n_fields; i++) {
        const bool is_f = d.kinds[i] == 'f';
        if (is_f ? (!f[i].f || f[i].u) : (!f[i].u || f[i].f)) return false;                  // the array of its kind, and no other
        s.field[i] = is_f ? (const uint32_t *)f[i].f : f[i].u;
    }
    s.on = s.field[d.on_field];
    return true;
}
}  // namespace

extern "C" {

int zh_span_merge_create(zh_ctx *ctx, uint32_t n_players, const zh_span_merge_source *a, const zh_span_merge_source *b, zh_span_merge **out) {
    ZH_GUARD(ctx);
    if (!ctx || !out || !merge_source_ok(a) || !merge_source_ok(b) || n_players > (1u << 31)) return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    zh_span_merge *m = new (std::nothrow) zh_span_merge();
    if (!m) return ZH_ERR_INVALID;
    memset(m, 0, sizeof *m);
    m->ctx = ctx; m->n = n_players; m->a = *a; m->b = *b;
    int rc = dev_alloc(&m->count, (size_t)n_players);
    if (!rc) rc = dev_alloc(&m->overflow, 1);
    if (!rc) rc = merge_alloc_tables(m, kMergeDefaultRows);
    if (!rc) rc = (int)hipMemsetAsync(m->overflow, 0, 4, ctx->stream);
    if (!rc && n_players) rc = (int)hipMemsetAsync(m->count, 0, (size_t)n_players * 4, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); merge_free(m); delete m; (void)hipGetLastError(); return rc; }
    *out = m;
    return ZH_OK;
}

int zh_span_merge_destroy(zh_span_merge *m) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m) return ZH_ERR_INVALID;
    if (!m->ctx->capturing) (void)hipStreamSynchronize(m->ctx->stream);
    merge_free(m);
    delete m;
    return ZH_OK;
}

int zh_span_merge_reserve(zh_span_merge *m, uint32_t max_rows) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || max_rows == 0) return ZH_ERR_INVALID;
    if (m->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    if (max_rows == m->rows) return ZH_OK;
    ZH_TRY(hipStreamSynchronize(m->ctx->stream));
    merge_free_tables(m);
    return merge_alloc_tables(m, max_rows);
}

int zh_span_merge_schedule(zh_span_merge *m, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in_a,
                           const zh_script_span_param *fields_a, const zh_script_span_table *in_b, const zh_script_span_param *fields_b) {
    ZH_GUARD(m ? m->ctx : nullptr);
    MergeArgs g;
    if (!m || max_spans == 0 || max_spans > m->rows || !merge_src(m->a, in_a, fields_a, g.a) || !merge_src(m->b, in_b, fields_b, g.b))
        return ZH_ERR_INVALID;
    if (m->n == 0) return ZH_OK;
    g.n = m->n; g.out_len = out_len; g.max_spans = max_spans;
    g.out = MergeOut{m->count, m->start, m->end, m->changed, m->words, (size_t)m->rows * m->n};
    g.overflow = m->overflow;
    ZH_LAUNCH(k_span_merge, dim3((m->n + kMergeBlock - 1) / kMergeBlock), dim3(kMergeBlock), 0, m->ctx->stream, g);
    return zh_launch_status();
}

int zh_span_merge_script_table(const zh_span_merge *m, uint32_t max_spans, zh_script_span_table *out) {
    if (!m || !out || max_spans == 0 || max_spans > m->rows) return ZH_ERR_INVALID;
    *out = zh_script_span_table{max_spans, 0, m->count, m->start, m->end, m->changed};
    return ZH_OK;
}
int zh_span_merge_span_param(const zh_span_merge *m, uint32_t field, zh_script_span_param *out) {
    if (!m || !out || field >= merge_fields(m)) return ZH_ERR_INVALID;
    const uint32_t na = m->a.n_fields, nb = m->b.n_fields;
    const bool is_f = field < na ? m->a.kinds[field] == 'f' : field < na + nb ? m->b.kinds[field - na] == 'f' : false;
    const uint32_t *w = m->words + (size_t)field * m->rows * m->n;
    *out = is_f ? zh_script_span_param{(const float *)w, nullptr} : zh_script_span_param{nullptr, w};
    return ZH_OK;
}

int zh_span_merge_overflows(zh_span_merge *m, uint64_t *out) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !out) return ZH_ERR_INVALID;
    uint32_t w = 0;
    int rc = zh_download(m->ctx, &w, m->overflow, 4);
    *out = w;
    return rc;
}

}  // extern "C"
