// saw_env.hip.h -- InnerInstrument of examples/example_subsong.zig (:24-68): a TriSawOsc of constant frequency times an Envelope
// whose three curves are cubed.  Two parts, as lead.hip.h: the state's layout as plain C++ (zh_saw_env_state <-> [word][voice]
// rows), and the lane (hipcc only): TriSawOscLane of voices.hip.h on its constant-frequency path and EnvLaneCubed of
// envelope.hip.h, untouched, under span_voice.hip.h's frame loop over one column.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"
#include "module_state.hip.h"

enum { SE_OSC_CNT = 0, SE_OSC_T, SE_ENV_STATE, SE_ENV_T, SE_ENV_LAST, SE_ENV_START, kSawEnvState };   // words per voice, [word][voice]

inline void se_pack(const zh_saw_env_state &s, uint32_t *w, size_t n, size_t v) {
    w[(size_t)SE_OSC_CNT * n + v] = s.osc.cnt; w[(size_t)SE_OSC_T * n + v] = zh_f32_bits(s.osc.t);
    env_pack(s.env, w + (size_t)SE_ENV_STATE * n + v, n);
}
inline void se_unpack(zh_saw_env_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.osc.cnt = w[(size_t)SE_OSC_CNT * n + v]; s.osc.t = zh_bits_f32(w[(size_t)SE_OSC_T * n + v]);
    s.env = env_unpack(w + (size_t)SE_ENV_STATE * n + v, n);
}
using SawEnvLayout = VoiceLayout<zh_saw_env_state, kSawEnvState, se_pack, se_unpack>;

#if defined(__HIPCC__)
#include "lead.hip.h"

// The lane contract of span_voice.hip.h (load_state / store_state, begin, frame, end).  `0.0f +` is the zang.zero of :51 followed by
// TriSawOsc's `+=`; where the TriSawOsc paints nothing (freq < 0 or above sample_rate / 8, TriSawOsc.zig:84-86) temps[0] stays
// the zero.  The Envelope adds to a zeroed temps[1] (:57-65) or leaves it (idle, or note_on while releasing: frame_masked's
// +0.0); zang.multiply (:66) then adds osc * env to EVERY frame of the sub-span.  The constant-frequency TriSawOsc never touches
// its f32 phase `t` (:37): it is carried through.
static_assert((int)ZH_SAW_ENV_SPAN_FREQ == LEAD_SPAN_FREQ && (int)ZH_SAW_ENV_SPAN_NOTE_ON == LEAD_SPAN_NOTE_ON &&
              (int)ZH_SAW_ENV_SPAN_FIELDS == LEAD_SPAN_FIELDS, "the leads' span fields");
struct SawEnvLane : LeadVoice<zh_saw_env_params, zh_saw_env_patch, 1> {
    using Layout = SawEnvLayout;
    TriSawOscLane osc;
    EnvLaneCubed env;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        const uint32_t *s = st + v;
        osc.cnt = s[(size_t)SE_OSC_CNT * N]; osc.t = zbits_f(s[(size_t)SE_OSC_T * N]);
        env.state = s[(size_t)SE_ENV_STATE * N]; env.t = zbits_f(s[(size_t)SE_ENV_T * N]);
        env.last_value = zbits_f(s[(size_t)SE_ENV_LAST * N]); env.start = zbits_f(s[(size_t)SE_ENV_START * N]);
        // a paint without a sub-span runs no frame; the fields begin() sets are given values all the same
        osc.sample_rate = 0.0f; osc.saw = true;
        osc.begin_const(1.0f, 0.0f, 0.0f);
        env.idle(ZH_CURVE_CUBED);
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        uint32_t *s = st + v;
        s[(size_t)SE_OSC_CNT * N] = osc.cnt; s[(size_t)SE_OSC_T * N] = zbits_u(osc.t);
        s[(size_t)SE_ENV_STATE * N] = env.state; s[(size_t)SE_ENV_T * N] = zbits_u(env.t);
        s[(size_t)SE_ENV_LAST * N] = zbits_u(env.last_value); s[(size_t)SE_ENV_START * N] = zbits_u(env.start);
    }
    __device__ __forceinline__ void begin(const Args &a, const Args::Span &s, bool nic) {
        const zh_saw_env_patch &p = a.patch;
        osc.begin_const(a.sample_rate, s.freq, p.color);               // :52-56: the per-paint prologue, at every sub-span
        env.sample_rate = a.sample_rate;                               // :58-65
        env.sustain_volume = p.sustain_volume;
        env.attack = CurveP{ZH_CURVE_CUBED, p.attack};
        env.decay = CurveP{ZH_CURVE_CUBED, p.decay};
        env.release = CurveP{ZH_CURVE_CUBED, p.release};
        env.note_on = s.note_on != 0;
        env.begin(nic);
    }
    __device__ __forceinline__ float frame(float &f) {
        f = 0.0f;                                                      // there is no second column
        float val = 0.0f;
        const bool painted = osc.frame_const(val);
        const float o = painted ? 0.0f + val : 0.0f;                   // :51-56
        const float e = env.frame_masked();                            // :57-65
        return o * e;                                                  // :66 (the product is rounded, then added)
    }
    __device__ __forceinline__ void end() {}
};
#endif   // __HIPCC__
