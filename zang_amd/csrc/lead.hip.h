// lead.hip.h -- the two monophonic leads of the reference's examples, which share one Params record (sample_rate, freq, note_on)
// and both paint two outputs, the voice and its frequency image (the oscilloscope sync):
//   porta    examples/example_portamento.zig Instrument :20-87: a sine whose frequency glides (Portamento), times an Envelope; it
//            carries a note-level bit across sub-spans (prev_note_on, :32, :51)
//   vibrato  examples/example_vibrato.zig Instrument :17-69: a pulse whose frequency a slow sine modulates, times a Gate
// Two parts:
//   the state layouts (zh_porta_state, zh_vibrato_state <-> [word][voice] rows) as plain C++, so that a stand-alone harness packs and
//   reads them back under ASan and UBSan (tests/cpp/lead_state_host.cpp);
//   the lanes (hipcc only): PortamentoLane, SineOscLane, PulseOscLane (its control-image path) of voices.hip.h and EnvLaneT of
//   envelope.hip.h, untouched, in the reference's stage order.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/zang_hip.h"

// ---- the states' layouts -----------------------------------------------------------------------------------------------
// words per voice, [word][voice], in the order of the structs
enum { PS_PORTA_T = 0, PS_PORTA_LAST, PS_PORTA_START, PS_ENV_STATE, PS_ENV_T, PS_ENV_LAST, PS_ENV_START, PS_OSC_T, PS_PREV_NOTE_ON, kPortaState };
enum { VS_VIB_T = 0, VS_OSC_CNT, kVibratoState };

inline uint32_t ls_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
inline float ls_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// voice v of n: struct -> rows (w = uint32_t[kPortaState * n]) and back
inline void ps_pack(const zh_porta_state &s, uint32_t *w, size_t n, size_t v) {
    w[(size_t)PS_PORTA_T * n + v] = ls_bits(s.porta.t); w[(size_t)PS_PORTA_LAST * n + v] = ls_bits(s.porta.last_value);
    w[(size_t)PS_PORTA_START * n + v] = ls_bits(s.porta.start);
    w[(size_t)PS_ENV_STATE * n + v] = s.env.state; w[(size_t)PS_ENV_T * n + v] = ls_bits(s.env.t);
    w[(size_t)PS_ENV_LAST * n + v] = ls_bits(s.env.last_value); w[(size_t)PS_ENV_START * n + v] = ls_bits(s.env.start);
    w[(size_t)PS_OSC_T * n + v] = ls_bits(s.osc.t);
    w[(size_t)PS_PREV_NOTE_ON * n + v] = s.prev_note_on;
}
inline void ps_unpack(zh_porta_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.porta.t = ls_float(w[(size_t)PS_PORTA_T * n + v]); s.porta.last_value = ls_float(w[(size_t)PS_PORTA_LAST * n + v]);
    s.porta.start = ls_float(w[(size_t)PS_PORTA_START * n + v]);
    s.env.state = w[(size_t)PS_ENV_STATE * n + v]; s.env.t = ls_float(w[(size_t)PS_ENV_T * n + v]);
    s.env.last_value = ls_float(w[(size_t)PS_ENV_LAST * n + v]); s.env.start = ls_float(w[(size_t)PS_ENV_START * n + v]);
    s.osc.t = ls_float(w[(size_t)PS_OSC_T * n + v]);
    s.prev_note_on = w[(size_t)PS_PREV_NOTE_ON * n + v];
}
// ... (w = uint32_t[kVibratoState * n])
inline void vs_pack(const zh_vibrato_state &s, uint32_t *w, size_t n, size_t v) {
    w[(size_t)VS_VIB_T * n + v] = ls_bits(s.vib.t);
    w[(size_t)VS_OSC_CNT * n + v] = s.osc.cnt;
}
inline void vs_unpack(zh_vibrato_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.vib.t = ls_float(w[(size_t)VS_VIB_T * n + v]);
    s.osc.cnt = w[(size_t)VS_OSC_CNT * n + v];
}
// what the generic host side (lead.hip) reads of a voice: its struct, its words, its converters
struct PortaLayout {
    using State = zh_porta_state;
    enum { kWords = kPortaState };
    static void pack(const State &s, uint32_t *w, size_t n, size_t v) { ps_pack(s, w, n, v); }
    static void unpack(State &s, const uint32_t *w, size_t n, size_t v) { ps_unpack(s, w, n, v); }
};
struct VibratoLayout {
    using State = zh_vibrato_state;
    enum { kWords = kVibratoState };
    static void pack(const State &s, uint32_t *w, size_t n, size_t v) { vs_pack(s, w, n, v); }
    static void unpack(State &s, const uint32_t *w, size_t n, size_t v) { vs_unpack(s, w, n, v); }
};

// ---- the lanes -------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "common.hip.h"
#include "zmath.hip.h"
#include "seq.hip.h"
#include "envelope.hip.h"
#include "voices.hip.h"

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
};

// A lead's lane: load_state / store_state, begin(args, freq, note_on, note_id_changed) = the prologue of Instrument.paint,
// frame(f) -> what is added to outputs[0], f = what is added to outputs[1], end() = its epilogue.  Every `0.0f +` is a zang.zero
// followed by a module's `+=`: -0.0 becomes +0.0.
struct PortaLane {
    using Patch = zh_porta_patch;
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
        env.sample_rate = 0.0f; env.sustain_volume = 0.0f; env.note_on = false;
        env.attack = env.decay = env.release = CurveP{ZH_CURVE_CUBED, 0.0f};
        env.mode = ENV_MODE_NONE; env.cur_tag = ZH_CURVE_CUBED; env.cur_step = env.cur_goal = env.cur_delta = 0.0f; env.m_painted = 0;
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        uint32_t *s = st + v;
        s[(size_t)PS_PORTA_T * N] = zbits_u(porta.t); s[(size_t)PS_PORTA_LAST * N] = zbits_u(porta.last); s[(size_t)PS_PORTA_START * N] = zbits_u(porta.st);
        s[(size_t)PS_ENV_STATE * N] = env.state; s[(size_t)PS_ENV_T * N] = zbits_u(env.t);
        s[(size_t)PS_ENV_LAST * N] = zbits_u(env.last_value); s[(size_t)PS_ENV_START * N] = zbits_u(env.start);
        s[(size_t)PS_OSC_T * N] = zbits_u(osc.t);
        s[(size_t)PS_PREV_NOTE_ON * N] = prev_note_on ? 1u : 0u;
    }
    __device__ __forceinline__ void begin(const LeadArgs<Patch> &a, float freq, bool note_on, bool nic) {
        const zh_porta_patch &p = a.patch;
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

struct VibratoLane {
    using Patch = zh_vibrato_patch;
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
    __device__ __forceinline__ void begin(const LeadArgs<Patch> &a, float freq_, bool note_on, bool) {
        const zh_vibrato_patch &p = a.patch;
        vib.begin(a.sample_rate, p.vib_hz);                                     // :47-51
        freq = freq_; depth = p.depth;                                          // :52-55
        osc.begin_ctrl(a.sample_rate, p.color);                                 // :58-62
        gate = note_on ? 1.0f : 0.0f;                                           // :63-66 (0 + 1.0, or the zeroed temp)
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

// every voice has ONE sub-span, the span itself, with its own note_id_changed: a table that holds no arrays (the plain
// paints of lead.hip and saw_env.hip)
struct LeadOneSpanP {
    struct U32 { uint32_t x; __device__ __forceinline__ uint32_t operator[](size_t) const { return x; } };
    struct Nic { BoolP b; __device__ __forceinline__ uint8_t operator[](size_t v) const { return b.get((uint32_t)v) ? 1 : 0; } };
    uint32_t K;
    U32 count, start, end;
    Nic nic;                                                           // kv = 0 * V + v
};

// frames [f0, f1) of one voice; `active` = false paints nothing.  outputs[0] goes through frame_loop, input-free.  The second
// column (O1): a ZERO_FIRST paint stores it frame by frame; an ADD paint hands the image to frame_loop as an INPUT, so that its
// rows are fetched a chunk ahead like the output's, and stores old + f -- frame_loop reads the rows of chunk k + 1 before chunk k
// is computed and a frame's own row before its body in the tail: a row is never read after it was written.  Inside a sub-span
// EVERY frame of both columns is added to, a +-0.0 addend included.
template <bool ZF, bool O1, class L>
__device__ __forceinline__ void lead_paint_frames(L &n, const Img &out, const Img &out1, uint32_t v, uint32_t f0, uint32_t f1, bool active) {
    constexpr int NIN = (O1 && !ZF) ? 1 : 0;
    const float *ins[1] = {out1.p};
    const size_t istr[1] = {out1.stride};
    const uint32_t voff = v * 4u;
    frame_loop<8, ZF, NIN>(out.p, v, out.stride, ins, istr, f0, f1, [&](uint32_t i, const float (&x)[1], float &val) ZH_INLINE_LAMBDA {
        float f = 0.0f;
        if (active) val = n.frame(f);
        if constexpr (O1) {
            if (ZF) zrow_store<1>(zrow_rsrc(out1.p, out1.stride, i), voff, 0, active ? 0.0f + f : 0.0f);
            else if (active) zrow_store<1>(zrow_rsrc(out1.p, out1.stride, i), voff, 0, x[0] + f);   // porta :85, vibrato :56
        }
        return active;
    });
}
#endif   // __HIPCC__
