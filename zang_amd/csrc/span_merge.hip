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
    StageRows out;
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kMergeBlock) k_span_merge(const MergeArgs g) {
    const uint32_t p = blockIdx.x * kMergeBlock + threadIdx.x;
    if (p >= g.n) return;
    const uint32_t dropped = merge_lane(g.a, g.b, g.out, g.n, p, g.out_len, g.max_spans);
    if (dropped) atomicAdd(g.overflow, dropped);
}
}  // namespace

struct zh_span_merge : zh_stage {                                     // words: [a.n_fields + b.n_fields + 3][rows][n]
    zh_span_merge_source a, b;
};

namespace {
void merge_free(zh_span_merge *m) { stage_free(m->tab); }
bool merge_source_ok(const zh_span_merge_source *s) {
    if (!s || s->n_fields == 0 || s->n_fields > kMergeMaxFields || s->on_field >= s->n_fields) return false;
    for (uint32_t i = 0; i < s->n_fields; i++)
        if (s->kinds[i] != 'f' && s->kinds[i] != 'u') return false;
    return s->kinds[s->on_field] == 'u';
}
// a source's table and field arrays -> the lane's view; false: something the schedule refuses
bool merge_src(const zh_span_merge_source &d, const zh_script_span_table *t, const zh_script_span_param *f, MergeSrc &s) {
    if (!stage_input_ok(t, true) || !f) return false;
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
    m->ctx = ctx; m->a = *a; m->b = *b;
    const int rc = stage_create(m, n_players, a->n_fields + b->n_fields + kMergeOwnFields, kMergeDefaultRows);
    if (rc) return stage_create_failed(m, merge_free, rc);
    *out = m;
    return ZH_OK;
}

int zh_span_merge_destroy(zh_span_merge *m) { ZH_GUARD(m ? m->ctx : nullptr); return stage_destroy(m, merge_free); }
int zh_span_merge_reserve(zh_span_merge *m, uint32_t max_rows) { ZH_GUARD(m ? m->ctx : nullptr); return stage_reserve(m, max_rows); }

int zh_span_merge_schedule(zh_span_merge *m, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in_a,
                           const zh_script_span_param *fields_a, const zh_script_span_table *in_b, const zh_script_span_param *fields_b) {
    ZH_GUARD(m ? m->ctx : nullptr);
    MergeArgs g;
    if (!stage_spans_ok(m, max_spans) || !merge_src(m->a, in_a, fields_a, g.a) || !merge_src(m->b, in_b, fields_b, g.b)) return ZH_ERR_INVALID;
    const uint32_t n = m->tab.n;
    if (n == 0) return ZH_OK;
    g.n = n; g.out_len = out_len; g.max_spans = max_spans;
    g.out = stage_rows(m);
    g.overflow = m->tab.overflow;
    ZH_LAUNCH(k_span_merge, dim3((n + kMergeBlock - 1) / kMergeBlock), dim3(kMergeBlock), 0, m->ctx->stream, g);
    return zh_launch_status();
}

int zh_span_merge_script_table(const zh_span_merge *m, uint32_t max_spans, zh_script_span_table *out) { return stage_script_table(m, max_spans, out); }
int zh_span_merge_span_param(const zh_span_merge *m, uint32_t field, zh_script_span_param *out) {
    if (!m) return ZH_ERR_INVALID;
    const uint32_t na = m->a.n_fields, nb = m->b.n_fields;
    return stage_span_param(m, field, field < na ? m->a.kinds[field] : field < na + nb ? m->b.kinds[field - na] : 'u', out);
}
int zh_span_merge_overflows(zh_span_merge *m, uint64_t *out) { ZH_GUARD(m ? m->ctx : nullptr); return stage_overflows(m, out); }

}  // extern "C"

