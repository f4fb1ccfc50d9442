// hard_square.hip -- HardSquareInstrument.paint (examples/modules.zig:269-288) plus the addScalarInto of
// examples/example_arpeggiator.zig:115 as ONE fused kernel per paint:
//   k_hard_square_spans<ZF, O1, HardSquareLane, TB>   the Trigger loop of Arpeggiator.paint (:106-116) for every voice from a span table
// on span_voice.hip.h's kernel body and host side: a lane per voice (hard_square.hip.h), contraction off, the PulseOsc's cnt
// loaded and stored once, span_walk's segments, two read-modify-write columns (the audio image and, O1, the frequency image).  The
// plain paint is the same kernel over a table of one sub-span per voice that holds no arrays.  Not built: a few-voice or
// frame-parallel form.
#include "hard_square.hip.h"

struct zh_hard_square : zh_voice {};

ZH_SPAN_VOICE_KERNEL(k_hard_square_spans)

extern "C" {

// init(): PulseOsc.init's cnt = 0 (modules.zig:262-267)
int zh_hard_square_create(zh_ctx *ctx, uint32_t n, zh_hard_square **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kHardSquareState, out); }
int zh_hard_square_destroy(zh_hard_square *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_hard_square_get_state(zh_hard_square *m, zh_hard_square_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    return voice_get_state<HardSquareLayout>(m, host);
}
int zh_hard_square_set_state(zh_hard_square *m, const zh_hard_square_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    return voice_set_state<HardSquareLayout>(m, host);
}
int zh_hard_square_paint(zh_hard_square *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                         const zh_hard_square_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps; (void)note_id_changed;                               // note_id_changed reaches no module of this voice
    return voice_paint<k_hard_square_spans_launch, HardSquareLane>(m, start, end, outputs, BoolP{0, nullptr}, p, flags);
}
int zh_hard_square_paint_spans(zh_hard_square *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps,
                               const zh_hard_square_params *p, const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) {
    ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint_spans<k_hard_square_spans_launch, HardSquareLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
