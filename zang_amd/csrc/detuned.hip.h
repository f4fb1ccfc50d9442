// detuned.hip.h -- the noise-warbled voice of examples/example_detuned.zig (OuterInstrument :103-169 over Instrument :31-101): a
// sawtooth whose frequency is warbled by low-passed white noise, enveloped, then low-passed again.  Two parts:
//   the state layout (zh_detuned_state <-> [word][voice] rows) as plain C++, so that a stand-alone harness packs and reads it back
//   under ASan and UBSan (tests/cpp/detuned_state_host.cpp);
//   the lane (hipcc only): NoiseLane, FilterLane x 2, TriSawOscLane (its control-image path) of voices.hip.h and EnvLaneT of
//   envelope.hip.h, untouched, in the reference's stage order.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"
#include "module_state.hip.h"

// ---- the state's layout ------------------------------------------------------------------------------------------------
// words per voice, [word][voice], in the order of zh_detuned_state; the generator's four u64 as (low, high) pairs.  The taps of
// zh_noise_state (`b`) are not held: white noise never reads them (Noise.zig:51) and the reference never writes them back (:68).
enum { DS_RNG = 0, DS_NF_L = 8, DS_NF_B, DS_OSC_CNT, DS_OSC_T, DS_ENV_STATE, DS_ENV_T, DS_ENV_LAST, DS_ENV_START, DS_MF_L, DS_MF_B, kDetunedState };

// voice v of n: struct -> rows (w = uint32_t[kDetunedState * n]) and back
inline void ds_pack(const zh_detuned_state &s, uint32_t *w, size_t n, size_t v) {
    for (int j = 0; j < 4; j++) {
        w[(size_t)(DS_RNG + 2 * j) * n + v] = (uint32_t)s.noise.r[j];
        w[(size_t)(DS_RNG + 2 * j + 1) * n + v] = (uint32_t)(s.noise.r[j] >> 32);
    }
    w[(size_t)DS_NF_L * n + v] = zh_f32_bits(s.noise_filter.l); w[(size_t)DS_NF_B * n + v] = zh_f32_bits(s.noise_filter.b);
    w[(size_t)DS_OSC_CNT * n + v] = s.osc.cnt; w[(size_t)DS_OSC_T * n + v] = zh_f32_bits(s.osc.t);
    env_pack(s.env, w + (size_t)DS_ENV_STATE * n + v, n);
    w[(size_t)DS_MF_L * n + v] = zh_f32_bits(s.main_filter.l); w[(size_t)DS_MF_B * n + v] = zh_f32_bits(s.main_filter.b);
}
inline void ds_unpack(zh_detuned_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));                                          // the taps, `reserved`
    for (int j = 0; j < 4; j++)
        s.noise.r[j] = (uint64_t)w[(size_t)(DS_RNG + 2 * j) * n + v] | ((uint64_t)w[(size_t)(DS_RNG + 2 * j + 1) * n + v] << 32);
    s.noise_filter.l = zh_bits_f32(w[(size_t)DS_NF_L * n + v]); s.noise_filter.b = zh_bits_f32(w[(size_t)DS_NF_B * n + v]);
    s.osc.cnt = w[(size_t)DS_OSC_CNT * n + v]; s.osc.t = zh_bits_f32(w[(size_t)DS_OSC_T * n + v]);
    s.env = env_unpack(w + (size_t)DS_ENV_STATE * n + v, n);
    s.main_filter.l = zh_bits_f32(w[(size_t)DS_MF_L * n + v]); s.main_filter.b = zh_bits_f32(w[(size_t)DS_MF_B * n + v]);
}
using DetunedLayout = VoiceLayout<zh_detuned_state, kDetunedState, ds_pack, ds_unpack>;

// ---- the lane --------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "common.hip.h"
#include "zmath.hip.h"
#include "seq.hip.h"
#include "envelope.hip.h"
#include "voices.hip.h"
#include "sample_kit.hip.h"        // ZkU32P

struct DetunedArgs {
    uint32_t V;
    uint32_t *state;                                                  // [kDetunedState][V]
    float sample_rate;
    zh_detuned_patch patch;
    F32P freq;
    BoolP note_on;
    ZkU32P mode;
    const float *sf;                                                  // the span arrays (ZH_DETUNED_SPAN_*), or NULL
    const uint32_t *sn, *sm;

    struct Span { float freq; uint32_t note_on, mode; };              // one sub-span's fields, as the span arrays hold them
    __device__ __forceinline__ Span defaults(uint32_t v) const { return Span{freq.get(v), note_on.get(v) ? 1u : 0u, mode.get(v)}; }
    __device__ __forceinline__ Span span(size_t kv, const Span &d) const { return Span{span_f(sf, kv, d.freq), span_u(sn, kv, d.note_on), span_u(sm, kv, d.mode)}; }
};

// the lane contract of span_voice.hip.h, device and host side
struct DetunedLane {
    using Params = zh_detuned_params;
    using Args = DetunedArgs;
    using Layout = DetunedLayout;
    static constexpr int kOutputs = 2;
    static constexpr int kFields = ZH_DETUNED_SPAN_FIELDS;
    static constexpr uint8_t kinds[ZH_DETUNED_SPAN_FIELDS] = {SPAN_F, SPAN_U, SPAN_U};
    static Args args(const zh_voice &m, const Params &p, const zh_script_span_param *sp) {
        return Args{m.n, m.state, p.sample_rate, p.patch, mk_f32(p.freq), mk_bool(p.note_on), ZkU32P{p.mode.value, p.mode.per_voice},
                    span_fa(sp, ZH_DETUNED_SPAN_FREQ), span_ua(sp, ZH_DETUNED_SPAN_NOTE_ON), span_ua(sp, ZH_DETUNED_SPAN_MODE)};
    }
    NoiseLane noise;
    FilterLane nf, mf;
    TriSawOscLane osc;
    EnvLaneCubed env;                                                 // all three curves are cubed (:81-83)
    float freq, wide_mul, volume;
    bool wide;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        const uint32_t *s = st + v;
        auto u64 = [&](int j) { return (uint64_t)s[(size_t)(DS_RNG + 2 * j) * N] | ((uint64_t)s[(size_t)(DS_RNG + 2 * j + 1) * N] << 32); };
        noise.r = ZXoshiro{u64(0), u64(1), u64(2), u64(3)};
        nf.l = zbits_f(s[(size_t)DS_NF_L * N]); nf.b = zbits_f(s[(size_t)DS_NF_B * N]);
        osc.cnt = s[(size_t)DS_OSC_CNT * N]; osc.t = zbits_f(s[(size_t)DS_OSC_T * N]);
        env.state = s[(size_t)DS_ENV_STATE * N]; env.t = zbits_f(s[(size_t)DS_ENV_T * N]);
        env.last_value = zbits_f(s[(size_t)DS_ENV_LAST * N]); env.start = zbits_f(s[(size_t)DS_ENV_START * N]);
        mf.l = zbits_f(s[(size_t)DS_MF_L * N]); mf.b = zbits_f(s[(size_t)DS_MF_B * N]);
        // a paint without a sub-span runs no frame; the fields begin() sets are given values all the same
        freq = wide_mul = volume = 0.0f; wide = false;
        nf.begin(ZH_FILTER_LOW_PASS, 0.0f, 0.0f); mf.begin(ZH_FILTER_LOW_PASS, 0.0f, 0.0f);
        osc.begin_ctrl(0.0f, 0.0f);
        env.idle(ZH_CURVE_CUBED);
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        uint32_t *s = st + v;
        const uint64_t r[4] = {noise.r.s0, noise.r.s1, noise.r.s2, noise.r.s3};
#pragma unroll
        for (int j = 0; j < 4; j++) { s[(size_t)(DS_RNG + 2 * j) * N] = (uint32_t)r[j]; s[(size_t)(DS_RNG + 2 * j + 1) * N] = (uint32_t)(r[j] >> 32); }
        s[(size_t)DS_NF_L * N] = zbits_u(nf.l); s[(size_t)DS_NF_B * N] = zbits_u(nf.b);
        s[(size_t)DS_OSC_CNT * N] = osc.cnt; s[(size_t)DS_OSC_T * N] = zbits_u(osc.t);
        s[(size_t)DS_ENV_STATE * N] = env.state; s[(size_t)DS_ENV_T * N] = zbits_u(env.t);
        s[(size_t)DS_ENV_LAST * N] = zbits_u(env.last_value); s[(size_t)DS_ENV_START * N] = zbits_u(env.start);
        s[(size_t)DS_MF_L * N] = zbits_u(mf.l); s[(size_t)DS_MF_B * N] = zbits_u(mf.b);
    }
    // the prologues of OuterInstrument.paint and Instrument.paint, in the order the stages run
    __device__ __forceinline__ void begin(const Args &a, const Args::Span &s, bool nic) {
        const zh_detuned_patch &p = a.patch;
        noise.begin();                                                                                  // :140
        nf.begin(ZH_FILTER_LOW_PASS, zcutoff_from_frequency(p.warble_hz, a.sample_rate), 0.0f);         // :142-150
        wide = (s.mode & 1u) == 0; wide_mul = p.warble_wide;                                            // :152-154
        freq = s.freq;                                                                                  // :63
        osc.begin_ctrl(a.sample_rate, p.color);                                                         // :68-72
        volume = p.volume;                                                                              // :76
        env.sample_rate = a.sample_rate;                                                                // :79-86
        env.sustain_volume = p.sustain_volume;
        env.attack = CurveP{ZH_CURVE_CUBED, p.attack};
        env.decay = CurveP{ZH_CURVE_CUBED, p.decay};
        env.release = CurveP{ZH_CURVE_CUBED, p.release};
        env.note_on = s.note_on != 0;
        env.begin(nic);
        mf.begin(ZH_FILTER_LOW_PASS, zcutoff_from_frequency(p.cutoff_hz, a.sample_rate), p.res);        // :90-99
    }
    // one frame: returns what is added to outputs[0]; f = what is added to outputs[1].  Every `0.0f +` is a zang.zero followed by
    // a module's `+=`: -0.0 becomes +0.0.
    __device__ __forceinline__ float frame(float &f) {
        const float n = 0.0f + noise.template frame<false>();                   // :139-140
        float w = 0.0f + nf.template frame<false, false>(n, 0.0f, 0.0f);        // :141-150
        if (wide) w = w * wide_mul;                                             // :152-154
        f = freq * zpowf_pos(2.0f, w);                                          // :61-65
        float o = 0.0f + osc.frame_ctrl(f);                                     // :67-72
        o = o * volume;                                                         // :76
        const float e = env.frame_masked();                                     // :78-86
        const float x = 0.0f + o * e;                                           // :87-88
        return mf.template frame<false, false>(x, 0.0f, 0.0f);                  // :90-99
    }
    __device__ __forceinline__ void end() { osc.end_ctrl(); }                   // TriSawOsc.zig:155
};
#endif   // __HIPCC__
