// dual.hip -- what one inner span of MainModule.paint does (examples/example_two.zig:109-138, :153) as ONE fused kernel per paint:
//   k_dual_spans<ZF, O1, DualLane, TB>   the merge loop of :101-151 for every voice from a span table (the merge stage's, span_merge.hip)
// on span_voice.hip.h's kernel body and host side: a lane per voice (dual.hip.h), contraction off, the state loaded and stored
// once, span_walk's segments, two read-modify-write columns (the audio image and, O1, the frequency image).  The plain paint is
// the same kernel over a table of one sub-span per voice that holds no arrays.  Not built: a few-voice or frame-parallel form
// (DESIGN.md).
#include "dual.hip.h"

struct zh_dual : zh_voice {};

ZH_SPAN_VOICE_KERNEL(k_dual_spans)

extern "C" {

int zh_dual_patch_default(zh_dual_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_dual_patch{0.025f, 0.1f, 1.0f, 0.5f};                      // :132-135
    return ZH_OK;
}
// init() :52-53: every word zero (idle is 0)
int zh_dual_create(zh_ctx *ctx, uint32_t n, zh_dual **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kDualState, out); }
int zh_dual_destroy(zh_dual *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_dual_get_state(zh_dual *m, zh_dual_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<DualLayout>(m, host); }
int zh_dual_set_state(zh_dual *m, const zh_dual_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<DualLayout>(m, host); }
int zh_dual_paint(zh_dual *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                  const zh_dual_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint<k_dual_spans_launch, DualLane>(m, start, end, outputs, mk_bool(note_id_changed), p, flags);
}
int zh_dual_paint_spans(zh_dual *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps,
                        const zh_dual_params *p, const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) {
    ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint_spans<k_dual_spans_launch, DualLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
