// curve_player.hip.h -- the curve voice of examples/example_curve.zig (CurvePlayer, :33-96): two Curves (modulator frequency,
// carrier frequency) drive a phase-modulated pair of SineOscs; no volume curve -- the carrier adds straight into outputs[0] -- and
// the carrier's frequency image goes to outputs[1].  Two parts:
//   the state's layout (zh_curve_player_state <-> [word][voice] rows) as plain C++, so that a stand-alone harness packs and reads
//   it back under ASan and UBSan (tests/cpp/curve_player_state_host.cpp);
//   the lane (hipcc only): CurveLane x 2 and SineOscLane x 2 of voices.hip.h, untouched, in the reference's stage order, and the
//   adapter that puts it under span_voice_frames.  The curves come from an effect kit (laser.hip.h: its layout, unchanged).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "laser.hip.h"

// ---- the state's layout ------------------------------------------------------------------------------------------------
// words per voice, [word][voice], in the order of zh_curve_player_state (example_curve.zig:41-44); a Curve's four words are
// t, current_song_note, current_song_note_offset, next_song_note (curve_pack)
enum { CP_CARRIER_CURVE = 0, CP_CARRIER_T = 4, CP_MODULATOR_CURVE = 5, CP_MODULATOR_T = 9, kCurvePlayerState = 10 };

// voice v of n: struct -> rows (w = uint32_t[kCurvePlayerState * n]) and back
inline void cp_pack(const zh_curve_player_state &s, uint32_t *w, size_t n, size_t v) {
    curve_pack(s.carrier_curve, w + (size_t)CP_CARRIER_CURVE * n + v, n);
    w[(size_t)CP_CARRIER_T * n + v] = zh_f32_bits(s.carrier.t);
    curve_pack(s.modulator_curve, w + (size_t)CP_MODULATOR_CURVE * n + v, n);
    w[(size_t)CP_MODULATOR_T * n + v] = zh_f32_bits(s.modulator.t);
}
inline void cp_unpack(zh_curve_player_state &s, const uint32_t *w, size_t n, size_t v) {
    s.carrier_curve = curve_unpack(w + (size_t)CP_CARRIER_CURVE * n + v, n);
    s.carrier.t = zh_bits_f32(w[(size_t)CP_CARRIER_T * n + v]);
    s.modulator_curve = curve_unpack(w + (size_t)CP_MODULATOR_CURVE * n + v, n);
    s.modulator.t = zh_bits_f32(w[(size_t)CP_MODULATOR_T * n + v]);
}
using CurvePlayerLayout = VoiceLayout<zh_curve_player_state, kCurvePlayerState, cp_pack, cp_unpack>;

// ---- the lane --------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct CurvePlayerArgs {
    uint32_t V;
    uint32_t *state;                                                  // [kCurvePlayerState][V]
    const zh_curve_node *nodes;                                       // the kit
    const LkEffectDesc *desc;
    uint32_t count, array_nodes;
    float sample_rate;
    F32P rel_freq;
    ZkU32P effect;
    const float *sf;                                                  // the span arrays (ZH_CURVE_PLAYER_SPAN_*), or NULL
    const uint32_t *se;

    struct Span { float rel_freq; uint32_t effect; };                 // one sub-span's fields, as the span arrays hold them
    __device__ __forceinline__ Span defaults(uint32_t v) const { return Span{rel_freq.get(v), effect.get(v)}; }
    __device__ __forceinline__ Span span(size_t kv, const Span &d) const { return Span{span_f(sf, kv, d.rel_freq), span_u(se, kv, d.effect)}; }
};

// One Curve's tables live in scratch memory (voices.hip.h CurveTable): they are written in begin() and read where a curve span
// ends, a few times per sub-span.
struct CurvePlayerTables { CurveTable m, c; };

// The lane contract of span_voice.hip.h: the host side whole; of the device side everything but begin() and frame(), which take
// the tables and the frame's index in its sub-span (CurvePlayerFrames below hands them in).
struct CurvePlayerLane {
    using Params = zh_curve_player_params;
    using Args = CurvePlayerArgs;
    using Layout = CurvePlayerLayout;
    static constexpr int kOutputs = 2;
    static constexpr int kFields = ZH_CURVE_PLAYER_SPAN_FIELDS;
    static constexpr uint8_t kinds[ZH_CURVE_PLAYER_SPAN_FIELDS] = {SPAN_F, SPAN_U};
    static Args args(const zh_voice &m, const Params &p, const zh_script_span_param *sp);   // curve_player.hip: it reads the kit's handle

    CurveLane cm, cc;
    SineOscLane om, oc;
    float mul;
    bool dead;                                                        // no such effect: this paint() touches nothing

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        LaserLane::load_curve(cc, st + CP_CARRIER_CURVE * N + v, N);
        oc.t = __builtin_bit_cast(float, st[CP_CARRIER_T * N + v]);
        LaserLane::load_curve(cm, st + CP_MODULATOR_CURVE * N + v, N);
        om.t = __builtin_bit_cast(float, st[CP_MODULATOR_T * N + v]);
        dead = true;
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        LaserLane::store_curve(cc, st + CP_CARRIER_CURVE * N + v, N);
        st[CP_CARRIER_T * N + v] = __builtin_bit_cast(uint32_t, oc.t);
        LaserLane::store_curve(cm, st + CP_MODULATOR_CURVE * N + v, N);
        st[CP_MODULATOR_T * N + v] = __builtin_bit_cast(uint32_t, om.t);
    }
    // Curve.paint's prologue for one curve of the kit, as LaserLane::begin_curve: the carried node (Curve.zig:142-148) is read at
    // nodes[offset + cur], inside the array for every index a paint can leave (the kit's zero tail); one that lies past it --
    // zh_curve_player_set_state only -- drops the carried node instead of reading outside the kit.
    __device__ __forceinline__ static void begin_curve(CurveLane &o, CurveTable &tb, const Args &a, const LkCurveDesc d, uint32_t out_len, bool nic) {
        if (!nic && o.cur < o.next && (uint64_t)d.offset + o.cur >= a.array_nodes) o.cur = o.next;
        o.begin(tb, a.sample_rate, d.function, a.nodes + d.offset, d.count, out_len, nic);
    }
    // CurvePlayer.paint's prologue (example_curve.zig:55-95), in the order the stages run
    __device__ __forceinline__ void begin(CurvePlayerTables &tb, const Args &a, const Args::Span &s, uint32_t out_len, bool nic) {
        dead = s.effect >= a.count;
        if (dead) return;
        const LkEffectDesc d = a.desc[s.effect];
        mul = s.rel_freq;                                                       // :63
        begin_curve(cm, tb.m, a, d.curve[LK_MODULATOR], out_len, nic);          // :66-70
        om.begin(a.sample_rate, 0.0f);                                          // :74-78
        begin_curve(cc, tb.c, a, d.curve[LK_CARRIER], out_len, nic);            // :81-85
        oc.begin(a.sample_rate, 0.0f);                                          // :88-92
    }
    // one frame, r = its index in the sub-span: returns what is added to outputs[0]; f = what is added to outputs[1].  Every
    // `0.0f +` is a zang.zero followed by a module's `+=`: -0.0 becomes +0.0; a frame a curve does not paint keeps the zero.  The
    // carrier has none: it adds into the output itself.
    __device__ __forceinline__ float frame(const CurvePlayerTables &tb, uint32_t r, float &f) {
        float x;
        const bool pm = cm.frame(tb.m, r, x);
        const float f_m = (pm ? 0.0f + x : 0.0f) * mul;                         // :65-71
        const float p = 0.0f + om.template frame<true>(f_m, 0.0f);              // :73-78
        const bool pc = cc.frame(tb.c, r, x);
        f = (pc ? 0.0f + x : 0.0f) * mul;                                       // :80-86
        return oc.template frame<true>(f, p);                                   // :88-92
    }
    __device__ __forceinline__ void end() {
        if (dead) return;
        om.end(); oc.end();                                                     // SineOsc.zig:40
    }
};

// what span_voice_frames walks: the lane, its tables and the running frame's index in its sub-span (frame_loop calls the body for
// consecutive frames in order)
struct CurvePlayerFrames {
    CurvePlayerLane &n;
    const CurvePlayerTables &tb;
    uint32_t r;
    __device__ __forceinline__ float frame(float &f) { return n.frame(tb, r++, f); }
};
#endif   // __HIPCC__
