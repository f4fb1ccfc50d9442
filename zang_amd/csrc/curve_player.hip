// curve_player.hip -- the curve voice of examples/example_curve.zig (:18-96) as ONE fused kernel per paint:
//   k_curve_player_spans<ZF, O1, TB>  MainModule's Trigger loop (:126-129) for every voice from a span table, on span_walk's
//                                     segments; CurvePlayer.paint (:55-95) is the same kernel over a table of one sub-span per voice
// Lane object, frame body and the state's layout: curve_player.hip.h; the frame loop over both columns, the handle with create /
// destroy / get_state / set_state and the two paints: span_voice.hip.h; the effect kit the voices play from: laser.hip.  The kernel
// stays the voice's own, as k_laser_spans: the curves' tables live in scratch and a frame's index counts from its sub-span's
// start.  O1 = outputs[1], the carrier's frequency image, is painted.  Not built: a few-voice form, frame ranges, a tolerant form.
#include "curve_player.hip.h"

// the kit's handle, token for token as laser.hip defines it (one definition in two translation units;
// tests/test_curve_player_host.py holds the two texts to each other)
struct zh_sfx_kit {
    zh_ctx *ctx;
    uint32_t n, array_nodes;
    zh_curve_node *nodes;                // the array of lk_pack
    LkEffectDesc *desc;
    std::vector<zh_sfx_effect> effects;  // the entries as zh_sfx_kit_effect hands them out: `nodes` point into the array
};

struct zh_curve_player : zh_voice {};

// the values of example_curve.zig:18-31 as {value, t}
static const zh_curve_node kCurveExample[9] = {
    {110.0f, 0.0f}, {55.0f, 1.5f}, {220.0f, 3.0f},                                                         // modulator_curve :27-31
    {440.0f, 0.0f}, {880.0f, 0.5f}, {110.0f, 1.0f}, {660.0f, 1.5f}, {330.0f, 2.0f}, {20.0f, 3.9f},         // carrier_curve :18-25
};

CurvePlayerArgs CurvePlayerLane::args(const zh_voice &m, const zh_curve_player_params &p, const zh_script_span_param *sp) {
    return CurvePlayerArgs{m.n, m.state, p.kit->nodes, p.kit->desc, p.kit->n, p.kit->array_nodes, p.sample_rate, mk_f32(p.rel_freq),
                           ZkU32P{p.effect.value, p.effect.per_voice}, span_fa(sp, ZH_CURVE_PLAYER_SPAN_REL_FREQ), span_ua(sp, ZH_CURVE_PLAYER_SPAN_EFFECT)};
}

// TB: SpanWalkP, or OneSpanP (zh_curve_player_paint).  Idle lanes of the last wave shadow voice 0 read-only and store nothing.
// The voice's words are loaded and stored once; the fields of a sub-span without span arrays are read once, before the walk.  A
// dead lane (no such effect) paints as a frame outside every sub-span does.
template <bool ZF, bool O1, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_curve_player_spans(const CurvePlayerArgs a, const TB tb, const Img out, const Img out1, uint32_t start,
                                                                  uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    CurvePlayerLane n;
    CurvePlayerTables ct;
    n.load_state(a.state, a.V, v);
    const CurvePlayerArgs::Span d = a.defaults(v);
    uint32_t s0 = start;                                             // the running sub-span's first frame
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA {
                           s0 = tb.start[kv];
                           n.begin(ct, a, a.span(kv, d), tb.end[kv] - s0, nic);
                       },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA {
                           if (!live) return;
                           CurvePlayerFrames fr{n, ct, f0 - s0};
                           span_voice_frames<ZF, O1>(fr, out, out1, v, f0, f1, active && !n.dead);
                       },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}
ZH_VOICE_LAUNCHER(k_curve_player_spans, (k_curve_player_spans<ZF, O1, TB>))

// a NULL kit or a kit of another context is refused before the kernel's arguments are read from it
static bool curve_player_kit_ok(const zh_curve_player *m, const zh_curve_player_params *p) {
    return !m || !p || (p->kit && p->kit->ctx == m->ctx);            // a NULL m or p: the paint's own check answers
}

extern "C" {

int zh_sfx_effect_curve_example(zh_sfx_effect *effect, zh_curve_node *nodes) {
    if (!effect || !nodes) return ZH_ERR_INVALID;
    memcpy(nodes, kCurveExample, sizeof(kCurveExample));
    effect->modulator = zh_sfx_curve{nodes, 3, ZH_CURVE_FN_SMOOTHSTEP};       // :66-70
    effect->carrier = zh_sfx_curve{nodes + 3, 6, ZH_CURVE_FN_SMOOTHSTEP};     // :81-85
    effect->volume = zh_sfx_curve{nullptr, 0, ZH_CURVE_FN_SMOOTHSTEP};        // the voice has none
    return ZH_OK;
}

// init() :46-53: every word zero
int zh_curve_player_create(zh_ctx *ctx, uint32_t n, zh_curve_player **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kCurvePlayerState, out); }
int zh_curve_player_destroy(zh_curve_player *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_curve_player_get_state(zh_curve_player *m, zh_curve_player_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    return voice_get_state<CurvePlayerLayout>(m, host);
}
int zh_curve_player_set_state(zh_curve_player *m, const zh_curve_player_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    return voice_set_state<CurvePlayerLayout>(m, host);
}

int zh_curve_player_paint(zh_curve_player *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                          const zh_curve_player_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    if (!curve_player_kit_ok(m, p)) return ZH_ERR_INVALID;
    return voice_paint<k_curve_player_spans_launch, CurvePlayerLane>(m, start, end, outputs, mk_bool(note_id_changed), p, flags);
}

int zh_curve_player_paint_spans(zh_curve_player *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps,
                                const zh_curve_player_params *p, const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) {
    ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    if (!curve_player_kit_ok(m, p)) return ZH_ERR_INVALID;
    return voice_paint_spans<k_curve_player_spans_launch, CurvePlayerLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
