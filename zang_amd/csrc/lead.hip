// lead.hip -- the two monophonic leads of the reference's examples as ONE fused kernel per paint, one template over both lanes:
//   k_lead_spans<ZF, O1, PortaLane, TB>    examples/example_portamento.zig: MainModule's Trigger loop (:119-128) over Instrument.paint (:43-86)
//   k_lead_spans<ZF, O1, VibratoLane, TB>  examples/example_vibrato.zig: the Trigger loop (:101-110) over Instrument.paint (:38-68)
// for every voice from a span table, on span_walk's segments.  The plain paints (zh_porta_paint, zh_vibrato_paint) are the same
// kernel over a table of one sub-span per voice that holds no arrays.  Lane objects and the states' layouts: lead.hip.h; the
// kernel body, the frame loop and the host side: span_voice.hip.h.  O1 = outputs[1], the frequency image, is painted.  Not built:
// a few-voice form, a tolerant form.
#include "lead.hip.h"

struct zh_porta : zh_voice {};
struct zh_vibrato : zh_voice {};

ZH_SPAN_VOICE_KERNEL(k_lead_spans)

extern "C" {

int zh_porta_patch_default(zh_porta_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_porta_patch{ZH_CURVE_CUBED, 0.5f, 0.025f, 0.1f, 1.0f, 0.5f};                     // :57, :68-71
    return ZH_OK;
}
// init(): every word zero (portamento :34-41, vibrato :30-36)
int zh_porta_create(zh_ctx *ctx, uint32_t n, zh_porta **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kPortaState, out); }
int zh_porta_destroy(zh_porta *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_porta_get_state(zh_porta *m, zh_porta_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<PortaLayout>(m, host); }
int zh_porta_set_state(zh_porta *m, const zh_porta_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<PortaLayout>(m, host); }
int zh_porta_paint(zh_porta *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                   const zh_porta_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint<k_lead_spans_launch, PortaLane>(m, start, end, outputs, mk_bool(note_id_changed), p, flags);
}
int zh_porta_paint_spans(zh_porta *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_porta_params *p,
                         const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint_spans<k_lead_spans_launch, PortaLane>(m, start, end, outputs, p, sp, table, flags);
}

int zh_vibrato_patch_default(zh_vibrato_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_vibrato_patch{4.0f, 0.02f, 0.5f};                                                // :49, :54, :61
    return ZH_OK;
}
int zh_vibrato_create(zh_ctx *ctx, uint32_t n, zh_vibrato **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kVibratoState, out); }
int zh_vibrato_destroy(zh_vibrato *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_vibrato_get_state(zh_vibrato *m, zh_vibrato_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<VibratoLayout>(m, host); }
int zh_vibrato_set_state(zh_vibrato *m, const zh_vibrato_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<VibratoLayout>(m, host); }
int zh_vibrato_paint(zh_vibrato *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                     const zh_vibrato_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint<k_lead_spans_launch, VibratoLane>(m, start, end, outputs, mk_bool(note_id_changed), p, flags);
}
int zh_vibrato_paint_spans(zh_vibrato *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_vibrato_params *p,
                           const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint_spans<k_lead_spans_launch, VibratoLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
