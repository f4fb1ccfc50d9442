// lead.hip -- the two monophonic leads of the reference's examples as ONE fused kernel per paint, one template over both lanes:
//   k_lead_spans<ZF, O1, PortaLane, TB>    examples/example_portamento.zig: MainModule's Trigger loop (:119-128) over Instrument.paint (:43-86)
//   k_lead_spans<ZF, O1, VibratoLane, TB>  examples/example_vibrato.zig: the Trigger loop (:101-110) over Instrument.paint (:38-68)
// for every voice from a span table, on span_walk's segments.  The plain paints (zh_porta_paint, zh_vibrato_paint) are the same
// kernel over a table of one sub-span per voice that holds no arrays.  Lane objects, frame bodies and the states' layouts:
// lead.hip.h.  O1 = outputs[1], the frequency image, is painted.  Not built: a few-voice form, a tolerant form.
#include "common.hip.h"
#include "span_walk.hip.h"
#include "lead.hip.h"
#include <vector>
#include <string.h>

struct zh_lead {
    zh_ctx *ctx;
    uint32_t n;
    uint32_t *state;                     // [L::Layout::kWords][n]
};
struct zh_porta : zh_lead {};
struct zh_vibrato : zh_lead {};

// TB: SpanWalkP, or the table of one sub-span per voice below.  Idle lanes of the last wave shadow voice 0 read-only and store nothing.
template <bool ZF, bool O1, class L, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_lead_spans(const LeadArgs<typename L::Patch> a, const TB tb, const Img out, const Img out1, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    L n;
    n.load_state(a.state, a.V, v);
    const float freq0 = a.freq.get(v);
    const uint32_t note_on0 = a.note_on.get(v) ? 1u : 0u;
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { n.begin(a, span_f(a.sf, kv, freq0), span_u(a.sn, kv, note_on0) != 0, nic); },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA { if (live) lead_paint_frames<ZF, O1>(n, out, out1, v, f0, f1, active); },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}
// span fields of both voices: ZH_PORTA_SPAN_* == ZH_VIBRATO_SPAN_*
static_assert((int)ZH_PORTA_SPAN_FREQ == (int)ZH_VIBRATO_SPAN_FREQ && (int)ZH_PORTA_SPAN_NOTE_ON == (int)ZH_VIBRATO_SPAN_NOTE_ON &&
              (int)ZH_PORTA_SPAN_FIELDS == (int)ZH_VIBRATO_SPAN_FIELDS, "the two leads share one Params record");
enum { LEAD_SPAN_FREQ = ZH_PORTA_SPAN_FREQ, LEAD_SPAN_NOTE_ON = ZH_PORTA_SPAN_NOTE_ON, LEAD_SPAN_FIELDS = ZH_PORTA_SPAN_FIELDS };

// what both paints check, and the kernel's arguments
template <class PARAMS, class PATCH>
static int lead_args(zh_lead *m, uint32_t start, uint32_t end, const zh_buf *outputs, const PARAMS *p, const zh_script_span_param *sp, LeadArgs<PATCH> &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    if (outputs[1].ptr && !buf_covers(outputs[1], m->n, end)) return ZH_ERR_INVALID;
    a = LeadArgs<PATCH>{m->n, m->state, p->sample_rate, p->patch, mk_f32(p->freq), mk_bool(p->note_on), span_fa(sp, LEAD_SPAN_FREQ), span_ua(sp, LEAD_SPAN_NOTE_ON)};
    return ZH_OK;
}

template <class L, class TB>
static void lead_launch(zh_lead *m, const LeadArgs<typename L::Patch> &a, const TB &tb, const zh_buf *outputs, uint32_t start, uint32_t end, uint32_t flags) {
    const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0, o1 = outputs[1].ptr != nullptr;
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]), out1 = o1 ? mk_img(outputs[1]) : Img{nullptr, 0};
    if (zf && o1) ZH_LAUNCH((k_lead_spans<true, true, L, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
    else if (zf) ZH_LAUNCH((k_lead_spans<true, false, L, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
    else if (o1) ZH_LAUNCH((k_lead_spans<false, true, L, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
    else ZH_LAUNCH((k_lead_spans<false, false, L, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
}

template <class M> static int lead_create(zh_ctx *ctx, uint32_t n, uint32_t words, M **out) {
    if (!ctx || !out) return ZH_ERR_INVALID;
    M *m = new (std::nothrow) M();
    if (!m) return ZH_ERR_INVALID;
    m->ctx = ctx; m->n = n; m->state = nullptr;
    int rc = dev_alloc(&m->state, (size_t)words * n);                   // init(): every word zero (portamento :34-41, vibrato :30-36)
    if (!rc && n) { hipError_t e = hipMemsetAsync(m->state, 0, (size_t)words * n * 4, ctx->stream); if (e != hipSuccess) rc = (int)e; }
    if (rc) { (void)hipFree(m->state); delete m; return rc; }
    *out = m;
    return ZH_OK;
}
template <class M> static int lead_destroy(M *m) {
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->state);
    delete m;
    return ZH_OK;
}
template <class LY> static int lead_get_state(zh_lead *m, typename LY::State *host) {
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)LY::kWords * n);
    int rc = zh_download(m->ctx, w.data(), m->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < n; v++) LY::unpack(host[v], w.data(), n, v);
    return ZH_OK;
}
template <class LY> static int lead_set_state(zh_lead *m, const typename LY::State *host) {
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)LY::kWords * n);
    for (size_t v = 0; v < n; v++) LY::pack(host[v], w.data(), n, v);
    return n ? zh_upload(m->ctx, m->state, w.data(), w.size() * 4) : ZH_OK;
}
template <class L, class PARAMS>
static int lead_paint(zh_lead *m, uint32_t start, uint32_t end, const zh_buf *outputs, zh_bool note_id_changed, const PARAMS *p, uint32_t flags) {
    LeadArgs<typename L::Patch> a;
    int rc = lead_args(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    const LeadOneSpanP tb{1, {1}, {start}, {end}, {mk_bool(note_id_changed)}};
    lead_launch<L>(m, a, tb, outputs, start, end, flags);
    return zh_launch_status();
}
template <class L, class PARAMS>
static int lead_paint_spans(zh_lead *m, uint32_t start, uint32_t end, const zh_buf *outputs, const PARAMS *p, const zh_script_span_param *sp,
                            const zh_script_span_table *table, uint32_t flags) {
    static const uint8_t kinds[LEAD_SPAN_FIELDS] = {SPAN_F, SPAN_U};
    LeadArgs<typename L::Patch> a;
    int rc = lead_args(m, start, end, outputs, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, kinds, LEAD_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    lead_launch<L>(m, a, mk_span_walk(table), outputs, start, end, flags);
    return zh_launch_status();
}

extern "C" {

int zh_porta_patch_default(zh_porta_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_porta_patch{ZH_CURVE_CUBED, 0.5f, 0.025f, 0.1f, 1.0f, 0.5f};                     // :57, :68-71
    return ZH_OK;
}
int zh_porta_create(zh_ctx *ctx, uint32_t n, zh_porta **out) { ZH_GUARD(ctx); return lead_create(ctx, n, kPortaState, out); }
int zh_porta_destroy(zh_porta *m) { ZH_GUARD(m ? m->ctx : nullptr); return lead_destroy(m); }
int zh_porta_get_state(zh_porta *m, zh_porta_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return lead_get_state<PortaLayout>(m, host); }
int zh_porta_set_state(zh_porta *m, const zh_porta_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return lead_set_state<PortaLayout>(m, host); }
int zh_porta_paint(zh_porta *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                   const zh_porta_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return lead_paint<PortaLane>(m, start, end, outputs, note_id_changed, p, flags);
}
int zh_porta_paint_spans(zh_porta *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_porta_params *p,
                         const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return lead_paint_spans<PortaLane>(m, start, end, outputs, p, sp, table, flags);
}

int zh_vibrato_patch_default(zh_vibrato_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_vibrato_patch{4.0f, 0.02f, 0.5f};                                                // :49, :54, :61
    return ZH_OK;
}
int zh_vibrato_create(zh_ctx *ctx, uint32_t n, zh_vibrato **out) { ZH_GUARD(ctx); return lead_create(ctx, n, kVibratoState, out); }
int zh_vibrato_destroy(zh_vibrato *m) { ZH_GUARD(m ? m->ctx : nullptr); return lead_destroy(m); }
int zh_vibrato_get_state(zh_vibrato *m, zh_vibrato_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return lead_get_state<VibratoLayout>(m, host); }
int zh_vibrato_set_state(zh_vibrato *m, const zh_vibrato_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return lead_set_state<VibratoLayout>(m, host); }
int zh_vibrato_paint(zh_vibrato *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                     const zh_vibrato_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return lead_paint<VibratoLane>(m, start, end, outputs, note_id_changed, p, flags);
}
int zh_vibrato_paint_spans(zh_vibrato *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_vibrato_params *p,
                           const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return lead_paint_spans<VibratoLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
