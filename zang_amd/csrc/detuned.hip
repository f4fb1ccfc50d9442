// detuned.hip -- the noise-warbled voice of examples/example_detuned.zig (:31-169) as ONE fused kernel per paint:
//   k_detuned<ZF, O1, NIC>                    OuterInstrument.paint for every voice, one lane per voice (:125-168 over :53-100)
//   k_detuned_spans<ZF, O1, DetunedLane, TB>  MainModule's Trigger loop (:213-222) for every voice from a span table, on span_walk's segments
// Lane object and the state's layout: detuned.hip.h; the span kernel's body, the frame loop and the host side: span_voice.hip.h.
// O1 = outputs[1], the frequency image, is painted.  Not built: a few-voice form (role waves, a wave per voice, frame ranges), a
// tolerant form.
#include "detuned.hip.h"

struct zh_detuned : zh_voice {};

// Noise.init for voice v (Noise.zig:26-29: the (first_seed + v)-th instance); everything else starts from zero (:45-51, :117-123)
__global__ void k_detuned_seed(uint32_t *st, uint32_t n, uint64_t first_seed) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    ZXoshiro r;
    zxoshiro_seed(r, first_seed + v);
    const uint64_t s[4] = {r.s0, r.s1, r.s2, r.s3};
    for (int j = 0; j < 4; j++) { st[(size_t)(DS_RNG + 2 * j) * n + v] = (uint32_t)s[j]; st[(size_t)(DS_RNG + 2 * j + 1) * n + v] = (uint32_t)(s[j] >> 32); }
}

template <bool ZF, bool O1, class NIC>
__global__ void __launch_bounds__(kSeqBlock) k_detuned(const DetunedArgs a, const NIC nic, const Img out, const Img out1, uint32_t start, uint32_t end) {
    const uint32_t v = blockIdx.x * kSeqBlock + threadIdx.x;
    if (v >= a.V) return;
    DetunedLane n;
    n.load_state(a.state, a.V, v);
    n.begin(a, a.defaults(v), nic.get(v));
    span_voice_frames<ZF, O1>(n, out, out1, v, start, end, true);
    n.end();
    n.store_state(a.state, a.V, v);
}
ZH_VOICE_LAUNCHER(k_detuned, (k_detuned<ZF, O1, TB>))      // TB: the type of note_id_changed

ZH_SPAN_VOICE_KERNEL(k_detuned_spans)

extern "C" {

int zh_detuned_patch_default(zh_detuned_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_detuned_patch{4.0f, 4.0f, 0.0f, 0.75f, 0.025f, 0.1f, 1.0f, 0.5f, 880.0f, 0.8f};   // :146, :153, :71, :76, :81-84, :95, :98
    return ZH_OK;
}

int zh_detuned_create(zh_ctx *ctx, uint32_t n, uint64_t first_seed, zh_detuned **out) { ZH_GUARD(ctx);
    int rc = voice_create(ctx, n, kDetunedState, out);
    if (rc) return rc;
    if (n) ZH_LAUNCH(k_detuned_seed, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (*out)->state, n, first_seed);
    return zh_launch_status();
}
int zh_detuned_destroy(zh_detuned *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_detuned_get_state(zh_detuned *m, zh_detuned_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<DetunedLayout>(m, host); }
int zh_detuned_set_state(zh_detuned *m, const zh_detuned_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<DetunedLayout>(m, host); }

// the dispatch row detuned_uniform_walk: the span kernel over the table of one sub-span per voice, or k_detuned
int zh_detuned_paint(zh_detuned *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                     const zh_detuned_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    DetunedArgs a;
    int rc = voice_args<DetunedLane>(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    const BoolP nic = mk_bool(note_id_changed);
    if (zh_form(ZF_DETUNED_UNIFORM_WALK) > 0) voice_launch<k_detuned_spans_launch, DetunedLane>(m, a, OneSpanP{1, {1}, {start}, {end}, {nic}}, outputs, start, end, flags);
    else voice_launch<k_detuned_launch, DetunedLane>(m, a, nic, outputs, start, end, flags);
    return zh_launch_status();
}

int zh_detuned_paint_spans(zh_detuned *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_detuned_params *p,
                           const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    return voice_paint_spans<k_detuned_spans_launch, DetunedLane>(m, start, end, outputs, p, sp, table, flags);
}

}  // extern "C"
