// saw_env.hip -- InnerInstrument.paint (examples/example_subsong.zig:43-67) as ONE fused kernel per paint:
//   k_saw_env_spans<ZF, false, SawEnvLane, TB>   the Trigger loop of SubtrackPlayer.paint (:135-143) for every voice from a span table
// on span_voice.hip.h's kernel body and host side: a lane per voice (saw_env.hip.h), contraction off, the state loaded and stored
// once, span_walk's segments, one read-modify-write column (SawEnvLane::kOutputs = 1: outputs[] has one entry, O1 is never built).
// The plain paint is the same kernel over a table of one sub-span per voice that holds no arrays.  Not built: a few-voice or
// frame-parallel form.
#include "saw_env.hip.h"

struct zh_saw_env : zh_voice {};

ZH_SPAN_VOICE_KERNEL(k_saw_env_spans)

extern "C" {

int zh_saw_env_patch_default(zh_saw_env_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_saw_env_patch{0.0f, 0.025f, 0.1f, 0.15f, 0.5f};            // :55, :60-63
    return ZH_OK;
}
// init() :36-41: every word zero (idle is 0)
int zh_saw_env_create(zh_ctx *ctx, uint32_t n, zh_saw_env **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kSawEnvState, out); }
int zh_saw_env_destroy(zh_saw_env *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_saw_env_get_state(zh_saw_env *m, zh_saw_env_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<SawEnvLayout>(m, host); }
int zh_saw_env_set_state(zh_saw_env *m, const zh_saw_env_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<SawEnvLayout>(m, host); }
int zh_saw_env_paint(zh_saw_env *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                     const zh_saw_env_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint<k_saw_env_spans_launch, SawEnvLane>(m, start, end, outputs, mk_bool(note_id_changed), p, flags);
}
int zh_saw_env_paint_spans(zh_saw_env *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps,
                           const zh_saw_env_params *p, const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) {
    ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint_spans<k_saw_env_spans_launch, SawEnvLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
