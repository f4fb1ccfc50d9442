// dual.hip.h -- the voice of examples/example_two.zig (MainModule.paint :109-138, :153): a TriSawOsc of constant frequency and
// color times an Envelope whose three curves are cubed, with the frequency image of :109 beside it.  One voice driven by two
// impulse streams: freq comes from one source, color from the other, note_on and note_id_changed from both (the merge stage,
// span_merge.hip).  Two parts, as saw_env.hip.h: the state's layout as plain C++ (zh_dual_state <-> [word][voice] rows), and the
// lane (hipcc only): TriSawOscLane of voices.hip.h on its constant-frequency path and EnvLaneCubed of envelope.hip.h, untouched,
// under span_voice.hip.h's frame loop over two columns.  A lane of its own: SawEnvLane is not shared, its kernels are untouched.
// One difference from the example: it multiplies over the whole buffer (:153), so a frame no inner span covers gets `+= 0 * 0`
// there (a -0.0 in the output becomes +0.0); the span-paint contract leaves such frames alone.  With ZH_PAINT_ZERO_FIRST, which
// the player uses, the two are identical.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"
#include "module_state.hip.h"

enum { DL_OSC_CNT = 0, DL_OSC_T, DL_ENV_STATE, DL_ENV_T, DL_ENV_LAST, DL_ENV_START, kDualState };   // words per voice, [word][voice]

inline void dl_pack(const zh_dual_state &s, uint32_t *w, size_t n, size_t v) {
    w[(size_t)DL_OSC_CNT * n + v] = s.osc.cnt; w[(size_t)DL_OSC_T * n + v] = zh_f32_bits(s.osc.t);
    env_pack(s.env, w + (size_t)DL_ENV_STATE * n + v, n);
}
inline void dl_unpack(zh_dual_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.osc.cnt = w[(size_t)DL_OSC_CNT * n + v]; s.osc.t = zh_bits_f32(w[(size_t)DL_OSC_T * n + v]);
    s.env = env_unpack(w + (size_t)DL_ENV_STATE * n + v, n);
}
using DualLayout = VoiceLayout<zh_dual_state, kDualState, dl_pack, dl_unpack>;

#if defined(__HIPCC__)
#include "common.hip.h"
#include "zmath.hip.h"
#include "seq.hip.h"
#include "envelope.hip.h"
#include "voices.hip.h"

struct DualArgs {
    uint32_t V;
    uint32_t *state;                                                  // [kDualState][V]
    float sample_rate;
    zh_dual_patch patch;
    F32P freq, color;
    BoolP note_on;
    const float *sf, *sc;                                             // the span arrays (ZH_DUAL_SPAN_*), or NULL
    const uint32_t *sn;

    struct Span { float freq, color; uint32_t note_on; };             // one sub-span's fields, as the span arrays hold them
    __device__ __forceinline__ Span defaults(uint32_t v) const { return Span{freq.get(v), color.get(v), note_on.get(v) ? 1u : 0u}; }
    __device__ __forceinline__ Span span(size_t kv, const Span &d) const {
        return Span{span_f(sf, kv, d.freq), span_f(sc, kv, d.color), span_u(sn, kv, d.note_on)};
    }
};

// The lane contract of span_voice.hip.h (load_state / store_state, begin, frame, end).  `0.0f +` is the zang.zero of :83 followed by
// TriSawOsc's `+=`; where the TriSawOsc paints nothing (freq < 0 or above sample_rate / 8, TriSawOsc.zig:84-86) temps[0] stays
// the zero.  The Envelope adds to a zeroed temps[1] (:84, :121-138) or leaves it (idle, or note_on while releasing: frame_masked's
// +0.0); zang.multiply (:153) then adds osc * env to EVERY frame of the sub-span.  The constant-frequency TriSawOsc never touches
// its f32 phase `t`: it is carried through.
struct DualLane {
    using Params = zh_dual_params;
    using Patch = zh_dual_patch;
    using Args = DualArgs;
    using Layout = DualLayout;
    static constexpr int kOutputs = 2;
    static constexpr int kFields = ZH_DUAL_SPAN_FIELDS;
    static constexpr uint8_t kinds[ZH_DUAL_SPAN_FIELDS] = {SPAN_F, SPAN_F, SPAN_U};
    static Args args(const zh_voice &m, const Params &p, const zh_script_span_param *sp) {
        return Args{m.n, m.state, p.sample_rate, p.patch, mk_f32(p.freq), mk_f32(p.color), mk_bool(p.note_on),
                    span_fa(sp, ZH_DUAL_SPAN_FREQ), span_fa(sp, ZH_DUAL_SPAN_COLOR), span_ua(sp, ZH_DUAL_SPAN_NOTE_ON)};
    }
    TriSawOscLane osc;
    EnvLaneCubed env;
    float freq;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        const uint32_t *s = st + v;
        osc.cnt = s[(size_t)DL_OSC_CNT * N]; osc.t = zbits_f(s[(size_t)DL_OSC_T * N]);
        env.state = s[(size_t)DL_ENV_STATE * N]; env.t = zbits_f(s[(size_t)DL_ENV_T * N]);
        env.last_value = zbits_f(s[(size_t)DL_ENV_LAST * N]); env.start = zbits_f(s[(size_t)DL_ENV_START * N]);
        // a paint without a sub-span runs no frame; the fields begin() sets are given values all the same
        freq = 0.0f;
        osc.sample_rate = 0.0f; osc.saw = true;
        osc.begin_const(1.0f, 0.0f, 0.0f);
        env.idle(ZH_CURVE_CUBED);
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        uint32_t *s = st + v;
        s[(size_t)DL_OSC_CNT * N] = osc.cnt; s[(size_t)DL_OSC_T * N] = zbits_u(osc.t);
        s[(size_t)DL_ENV_STATE * N] = env.state; s[(size_t)DL_ENV_T * N] = zbits_u(env.t);
        s[(size_t)DL_ENV_LAST * N] = zbits_u(env.last_value); s[(size_t)DL_ENV_START * N] = zbits_u(env.start);
    }
    __device__ __forceinline__ void begin(const Args &a, const Args::Span &s, bool nic) {
        const zh_dual_patch &p = a.patch;
        osc.begin_const(a.sample_rate, s.freq, s.color);               // :110-120: the per-paint prologue, at every sub-span
        freq = s.freq;
        env.sample_rate = a.sample_rate;                               // :121-138
        env.sustain_volume = p.sustain_volume;
        env.attack = CurveP{ZH_CURVE_CUBED, p.attack};
        env.decay = CurveP{ZH_CURVE_CUBED, p.decay};
        env.release = CurveP{ZH_CURVE_CUBED, p.release};
        env.note_on = s.note_on != 0;
        env.begin(nic);
    }
    __device__ __forceinline__ float frame(float &f) {
        f = freq;                                                      // :109
        float val = 0.0f;
        const bool painted = osc.frame_const(val);
        const float o = painted ? 0.0f + val : 0.0f;                   // :83, :110-120
        const float e = env.frame_masked();                            // :84, :121-138
        return o * e;                                                  // :153 (the product is rounded, then added)
    }
    __device__ __forceinline__ void end() {}
};
#endif   // __HIPCC__
