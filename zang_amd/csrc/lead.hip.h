// lead.hip.h -- the two monophonic leads of the reference's examples, which share one Params record (sample_rate, freq, note_on)
// and both paint two outputs, the voice and its frequency image (the oscilloscope sync):
//   porta    examples/example_portamento.zig Instrument :20-87: a sine whose frequency glides (Portamento), times an Envelope; it
//            carries a note-level bit across sub-spans (prev_note_on, :32, :51)
//   vibrato  examples/example_vibrato.zig Instrument :17-69: a pulse whose frequency a slow sine modulates, times a Gate
// Two parts:
//   the state layouts (zh_porta_state, zh_vibrato_state <-> [word][voice] rows) as plain C++, so that a stand-alone harness packs and
//   reads them back under ASan and UBSan (tests/cpp/lead_state_host.cpp);
//   the lanes (hipcc only): PortamentoLane, SineOscLane, PulseOscLane (its control-image path) of voices.hip.h and EnvLaneT of
//   envelope.hip.h, untouched, in the reference's stage order; and LeadArgs / LeadVoice, the argument block and the host-side
//   traits of every voice with this Params record (hard_square.hip.h and saw_env.hip.h too).  The kernel and the host side they
//   plug into: span_voice.hip.h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"
#include "module_state.hip.h"

// ---- the states' layouts -----------------------------------------------------------------------------------------------
// words per voice, [word][voice], in the order of the structs
enum { PS_PORTA_T = 0, PS_PORTA_LAST, PS_PORTA_START, PS_ENV_STATE, PS_ENV_T, PS_ENV_LAST, PS_ENV_START, PS_OSC_T, PS_PREV_NOTE_ON, kPortaState };
enum { VS_VIB_T = 0, VS_OSC_CNT, kVibratoState };

// voice v of n: struct -> rows (w = uint32_t[kPortaState * n]) and back
inline void ps_pack(const zh_porta_state &s, uint32_t *w, size_t n, size_t v) {
    porta_pack(s.porta, w + (size_t)PS_PORTA_T * n + v, n);
    env_pack(s.env, w + (size_t)PS_ENV_STATE * n + v, n);
    w[(size_t)PS_OSC_T * n + v] = zh_f32_bits(s.osc.t);
    w[(size_t)PS_PREV_NOTE_ON * n + v] = s.prev_note_on;
}
inline void ps_unpack(zh_porta_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.porta = porta_unpack(w + (size_t)PS_PORTA_T * n + v, n);
    s.env = env_unpack(w + (size_t)PS_ENV_STATE * n + v, n);
    s.osc.t = zh_bits_f32(w[(size_t)PS_OSC_T * n + v]);
    s.prev_note_on = w[(size_t)PS_PREV_NOTE_ON * n + v];
}
// ... (w = uint32_t[kVibratoState * n])
inline void vs_pack(const zh_vibrato_state &s, uint32_t *w, size_t n, size_t v) {
    w[(size_t)VS_VIB_T * n + v] = zh_f32_bits(s.vib.t);
    w[(size_t)VS_OSC_CNT * n + v] = s.osc.cnt;
}
inline void vs_unpack(zh_vibrato_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.vib.t = zh_bits_f32(w[(size_t)VS_VIB_T * n + v]);
    s.osc.cnt = w[(size_t)VS_OSC_CNT * n + v];
}
using PortaLayout = VoiceLayout<zh_porta_state, kPortaState, ps_pack, ps_unpack>;
using VibratoLayout = VoiceLayout<zh_vibrato_state, kVibratoState, vs_pack, vs_unpack>;

// ---- the lanes -------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "common.hip.h"
#include "zmath.hip.h"
#include "seq.hip.h"
#include "envelope.hip.h"
#include "voices.hip.h"

// the span fields of every voice with this Params record: ZH_PORTA_SPAN_* == ZH_VIBRATO_SPAN_* == ZH_HARD_SQUARE_SPAN_* == ZH_SAW_ENV_SPAN_*
static_assert((int)ZH_PORTA_SPAN_FREQ == (int)ZH_VIBRATO_SPAN_FREQ && (int)ZH_PORTA_SPAN_NOTE_ON == (int)ZH_VIBRATO_SPAN_NOTE_ON &&
              (int)ZH_PORTA_SPAN_FIELDS == (int)ZH_VIBRATO_SPAN_FIELDS, "the two leads share one Params record");
enum { LEAD_SPAN_FREQ = ZH_PORTA_SPAN_FREQ, LEAD_SPAN_NOTE_ON = ZH_PORTA_SPAN_NOTE_ON, LEAD_SPAN_FIELDS = ZH_PORTA_SPAN_FIELDS };

template <class PATCH>
struct LeadArgs {
    uint32_t V;
    uint32_t *state;                                                  // [kWords][V]
    float sample_rate;
    PATCH patch;
    F32P freq;
    BoolP note_on;
    const float *sf;                                                  // the span arrays (ZH_<X>_SPAN_*), or NULL
    const uint32_t *sn;

    struct Span { float freq; uint32_t note_on; };                    // one sub-span's fields, as the span arrays hold them
    __device__ __forceinline__ Span defaults(uint32_t v) const { return Span{freq.get(v), note_on.get(v) ? 1u : 0u}; }
    __device__ __forceinline__ Span span(size_t kv, const Span &d) const { return Span{span_f(sf, kv, d.freq), span_u(sn, kv, d.note_on)}; }
};

// What span_voice.hip.h's host side reads of a lane with this Params record (sample_rate, freq, note_on; `patch` where the voice has
// constants): OUTS columns, the two span fields.
template <class PARAMS, class PATCH, int OUTS>
struct LeadVoice {
    using Params = PARAMS;
    using Patch = PATCH;
    using Args = LeadArgs<PATCH>;
    static constexpr int kOutputs = OUTS;
    static constexpr int kFields = LEAD_SPAN_FIELDS;
    static constexpr uint8_t kinds[LEAD_SPAN_FIELDS] = {SPAN_F, SPAN_U};
    static Args args(const zh_voice &m, const PARAMS &p, const PATCH &patch, const zh_script_span_param *sp) {
        return Args{m.n, m.state, p.sample_rate, patch, mk_f32(p.freq), mk_bool(p.note_on), span_fa(sp, LEAD_SPAN_FREQ), span_ua(sp, LEAD_SPAN_NOTE_ON)};
    }
    static Args args(const zh_voice &m, const PARAMS &p, const zh_script_span_param *sp) { return args(m, p, p.patch, sp); }
};

// A lead's lane (the contract: span_voice.hip.h): begin(args, {freq, note_on}, note_id_changed) = the prologue of
// Instrument.paint, frame(f) -> what is added to outputs[0], f = what is added to outputs[1], end() = its epilogue.  Every
// `0.0f +` is a zang.zero followed by a module's `+=`: -0.0 becomes +0.0.
struct PortaLane : LeadVoice<zh_porta_params, zh_porta_patch, 2> {
    using Layout = PortaLayout;
    PortamentoLane porta;
    EnvLaneCubed env;                                                 // all three curves are cubed (:68-70)
    SineOscLane osc;
    bool prev_note_on, cur_note_on;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        const uint32_t *s = st + v;
        porta.t = zbits_f(s[(size_t)PS_PORTA_T * N]); porta.last = zbits_f(s[(size_t)PS_PORTA_LAST * N]); porta.st = zbits_f(s[(size_t)PS_PORTA_START * N]);
        env.state = s[(size_t)PS_ENV_STATE * N]; env.t = zbits_f(s[(size_t)PS_ENV_T * N]);
        env.last_value = zbits_f(s[(size_t)PS_ENV_LAST * N]); env.start = zbits_f(s[(size_t)PS_ENV_START * N]);
        osc.t = zbits_f(s[(size_t)PS_OSC_T * N]);
        prev_note_on = s[(size_t)PS_PREV_NOTE_ON * N] != 0;
        // a paint without a sub-span runs no frame; the fields begin() sets are given values all the same
        cur_note_on = prev_note_on;
        porta.goal = porta.t_step = 0.0f; porta.tag = ZH_CURVE_INSTANTANEOUS; porta.flat = true;
        osc.t_step = osc.inv_sr = 0.0f;
        env.idle(ZH_CURVE_CUBED);
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        uint32_t *s = st + v;
        s[(size_t)PS_PORTA_T * N] = zbits_u(porta.t); s[(size_t)PS_PORTA_LAST * N] = zbits_u(porta.last); s[(size_t)PS_PORTA_START * N] = zbits_u(porta.st);
        s[(size_t)PS_ENV_STATE * N] = env.state; s[(size_t)PS_ENV_T * N] = zbits_u(env.t);
        s[(size_t)PS_ENV_LAST * N] = zbits_u(env.last_value); s[(size_t)PS_ENV_START * N] = zbits_u(env.start);
        s[(size_t)PS_OSC_T * N] = zbits_u(osc.t);
        s[(size_t)PS_PREV_NOTE_ON * N] = prev_note_on ? 1u : 0u;
    }
    __device__ __forceinline__ void begin(const Args &a, const Args::Span &s, bool nic) {
        const zh_porta_patch &p = a.patch;
        const float freq = s.freq;
        const bool note_on = s.note_on != 0;
        porta.begin(a.sample_rate, p.glide_curve, p.glide, freq, note_on, prev_note_on, nic);             // :55-61
        env.sample_rate = a.sample_rate;                                                                  // :65-73
        env.sustain_volume = p.sustain_volume;
        env.attack = CurveP{ZH_CURVE_CUBED, p.attack};
        env.decay = CurveP{ZH_CURVE_CUBED, p.decay};
        env.release = CurveP{ZH_CURVE_CUBED, p.release};
        env.note_on = note_on;
        env.begin(!prev_note_on && note_on);                                                              // :65: only when every key was up
        osc.begin(a.sample_rate, 0.0f);                                                                   // :76-80 the frequency-buffer path
        cur_note_on = note_on;
    }
    __device__ __forceinline__ float frame(float &f) {
        f = 0.0f + porta.frame();                                               // :53-61
        const float e = env.frame_masked();                                     // :63-73
        const float s = 0.0f + osc.template frame<true>(f, 0.0f);               // :75-80
        return e * s;                                                           // :82 (the product is rounded, then added)
    }
    __device__ __forceinline__ void end() { osc.end(); prev_note_on = cur_note_on; }   // SineOsc.zig:40, then the defer of :51
};

struct VibratoLane : LeadVoice<zh_vibrato_params, zh_vibrato_patch, 2> {
    using Layout = VibratoLayout;
    SineOscLane vib;
    PulseOscLane osc;
    float freq, depth, gate;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        vib.t = zbits_f(st[(size_t)VS_VIB_T * N + v]);
        osc.cnt = st[(size_t)VS_OSC_CNT * N + v];
        freq = depth = gate = 0.0f;
        vib.begin(1.0f, 0.0f);
        osc.begin_ctrl(1.0f, 0.5f);
        osc.bad = false;
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        st[(size_t)VS_VIB_T * N + v] = zbits_u(vib.t);
        st[(size_t)VS_OSC_CNT * N + v] = osc.cnt;
    }
    // note_id_changed reaches no module of this voice (SineOsc, PulseOsc and Gate ignore it)
    __device__ __forceinline__ void begin(const Args &a, const Args::Span &s, bool) {
        const zh_vibrato_patch &p = a.patch;
        vib.begin(a.sample_rate, p.vib_hz);                                     // :47-51
        freq = s.freq; depth = p.depth;                                         // :52-55
        osc.begin_ctrl(a.sample_rate, p.color);                                 // :58-62
        gate = s.note_on != 0 ? 1.0f : 0.0f;                                       // :63-66 (0 + 1.0, or the zeroed temp)
    }
    __device__ __forceinline__ float frame(float &f) {
        const float m = 0.0f + vib.template frame<false>(0.0f, 0.0f);           // :46-51
        const float dm = depth * m;                                             // :54: three roundings, never fused
        const float one = 1.0f + dm;
        f = freq * one;
        float val = 0.0f;
        const bool painted = osc.frame_ctrl(f, val);                            // :57-62: out of range paints nothing
        const float o = painted ? 0.0f + val : 0.0f;
        return o * gate;                                                        // :67
    }
    __device__ __forceinline__ void end() { vib.end(); }                        // SineOsc.zig:40
};
#endif   // __HIPCC__
