// laser.hip.h -- the sound-effect voice of examples/example_laser.zig (LaserPlayer, :40-117): three Curves (modulator frequency,
// carrier frequency, volume) drive a phase-modulated pair of SineOscs.  Two parts:
//   the state's layout (zh_laser_state <-> [word][voice] rows) and the layout of an effect kit (zh_sfx_kit: K triples of curves, all nodes in one device array beside a descriptor table), as
//   plain C++ so that a stand-alone harness packs and reads it back under ASan and UBSan (tests/cpp/sfx_kit_host.cpp);
//   the lane (hipcc only): CurveLane x 3 and SineOscLane x 2 of voices.hip.h, untouched, in the reference's stage order.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"
#include "module_state.hip.h"

// ---- the state's layout ------------------------------------------------------------------------------------------------
// words per voice, [word][voice], in the order of zh_laser_state (example_laser.zig:51-55); a Curve's four words are
// t, current_song_note, current_song_note_offset, next_song_note (module_state.hip.h curve_pack)
enum { LS_CARRIER_CURVE = 0, LS_CARRIER_T = 4, LS_MODULATOR_CURVE = 5, LS_MODULATOR_T = 9, LS_VOLUME_CURVE = 10, kLaserState = 14 };

// voice v of n: struct -> rows (w = uint32_t[kLaserState * n]) and back
inline void lz_pack(const zh_laser_state &s, uint32_t *w, size_t n, size_t v) {
    curve_pack(s.carrier_curve, w + (size_t)LS_CARRIER_CURVE * n + v, n);
    w[(size_t)LS_CARRIER_T * n + v] = zh_f32_bits(s.carrier.t);
    curve_pack(s.modulator_curve, w + (size_t)LS_MODULATOR_CURVE * n + v, n);
    w[(size_t)LS_MODULATOR_T * n + v] = zh_f32_bits(s.modulator.t);
    curve_pack(s.volume_curve, w + (size_t)LS_VOLUME_CURVE * n + v, n);
}
inline void lz_unpack(zh_laser_state &s, const uint32_t *w, size_t n, size_t v) {
    s.carrier_curve = curve_unpack(w + (size_t)LS_CARRIER_CURVE * n + v, n);
    s.carrier.t = zh_bits_f32(w[(size_t)LS_CARRIER_T * n + v]);
    s.modulator_curve = curve_unpack(w + (size_t)LS_MODULATOR_CURVE * n + v, n);
    s.modulator.t = zh_bits_f32(w[(size_t)LS_MODULATOR_T * n + v]);
    s.volume_curve = curve_unpack(w + (size_t)LS_VOLUME_CURVE * n + v, n);
}
using LaserLayout = VoiceLayout<zh_laser_state, kLaserState, lz_pack, lz_unpack>;

// ---- the kit's layout ------------------------------------------------------------------------------------------------
// Effect i's curves lie one after the other (modulator, carrier, volume), the effects in the order given.  After the last
// node come as many ZERO nodes as the kit's longest curve has: a Curve reads the node it carried over from the previous
// paint at the index that paint left, counted from the first node of the curve it plays now (zh_curve_module: "whatever
// curve_len is now"), and an index that a paint of ANY curve of the kit can leave is below that length -- so the read stays
// inside the array when a sub-span switches to a shorter curve without note_id_changed.
struct LkCurveDesc { uint32_t offset, count, function; };             // nodes [offset, offset + count) of the array; ZH_CURVE_FN_*
struct LkEffectDesc { LkCurveDesc curve[3]; };                        // in paint order (example_laser.zig:78-113)
enum { LK_MODULATOR = 0, LK_CARRIER = 1, LK_VOLUME = 2 };

inline const zh_sfx_curve &lk_curve(const zh_sfx_effect &e, int c) { return c == LK_MODULATOR ? e.modulator : c == LK_CARRIER ? e.carrier : e.volume; }

// Fills desc[n] from effects[n] and returns the array's length, tail included, in *array_nodes; ZH_ERR_INVALID for what
// zh_sfx_kit_create refuses.
inline int lk_describe(const zh_sfx_effect *effects, uint32_t n, LkEffectDesc *desc, size_t *array_nodes) {
    if (!effects || n == 0) return ZH_ERR_INVALID;
    uint64_t at = 0;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            const zh_sfx_curve &k = lk_curve(effects[i], c);
            if (k.function > ZH_CURVE_FN_SMOOTHSTEP || (k.count && !k.nodes)) return ZH_ERR_INVALID;
            if (at + k.count > 0x7fffffffull) return ZH_ERR_INVALID;                 // offsets and the tail stay 32-bit
            desc[i].curve[c] = LkCurveDesc{(uint32_t)at, k.count, k.function};
            at += k.count;
            longest = k.count > longest ? k.count : longest;
        }
    *array_nodes = (size_t)(at + longest);
    return ZH_OK;
}
// The array of lk_describe's layout from the effects' HOST nodes; the tail is zero.
inline void lk_pack(const zh_sfx_effect *effects, uint32_t n, const LkEffectDesc *desc, zh_curve_node *array, size_t array_nodes) {
    for (size_t j = 0; j < array_nodes; j++) array[j] = zh_curve_node{0.0f, 0.0f};
    for (uint32_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            const zh_sfx_curve &k = lk_curve(effects[i], c);
            if (k.count) memcpy(array + desc[i].curve[c].offset, k.nodes, (size_t)k.count * sizeof(zh_curve_node));
        }
}

// ---- the lane --------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "common.hip.h"
#include "seq.hip.h"
#include "voices.hip.h"
#include "sample_kit.hip.h"        // ZkU32P

struct LaserArgs {
    uint32_t V;
    uint32_t *state;                                                  // [kLaserState][V]
    const zh_curve_node *nodes;                                       // the kit
    const LkEffectDesc *desc;
    uint32_t count, array_nodes;
    float sample_rate;
    F32P freq_mul, carrier_mul, modulator_mul, modulator_rad;
    ZkU32P effect;
    const float *sf, *sc, *sm, *sr;                                   // the span arrays (ZH_LASER_SPAN_*), or NULL
    const uint32_t *se;
};

// One Curve's three tables live in scratch memory (voices.hip.h CurveTable): they are written in begin() and read where a curve
// span ends, a few times per sub-span.
struct LaserTables { CurveTable m, c, v; };

struct LaserLane {
    CurveLane cm, cc, cv;
    SineOscLane om, oc;
    float mul_m, mul_c, rad;
    bool dead;                                                        // no such effect: this paint() touches nothing

    __device__ __forceinline__ static void load_curve(CurveLane &o, const uint32_t *s, size_t N) {
        o.t = __builtin_bit_cast(float, s[0]); o.cur = s[N]; o.off = (int32_t)s[2 * N]; o.next = s[3 * N];
    }
    __device__ __forceinline__ static void store_curve(const CurveLane &o, uint32_t *s, size_t N) {
        s[0] = __builtin_bit_cast(uint32_t, o.t); s[N] = o.cur; s[2 * N] = (uint32_t)o.off; s[3 * N] = o.next;
    }
    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        load_curve(cc, st + LS_CARRIER_CURVE * N + v, N);
        oc.t = __builtin_bit_cast(float, st[LS_CARRIER_T * N + v]);
        load_curve(cm, st + LS_MODULATOR_CURVE * N + v, N);
        om.t = __builtin_bit_cast(float, st[LS_MODULATOR_T * N + v]);
        load_curve(cv, st + LS_VOLUME_CURVE * N + v, N);
        dead = true;
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        store_curve(cc, st + LS_CARRIER_CURVE * N + v, N);
        st[LS_CARRIER_T * N + v] = __builtin_bit_cast(uint32_t, oc.t);
        store_curve(cm, st + LS_MODULATOR_CURVE * N + v, N);
        st[LS_MODULATOR_T * N + v] = __builtin_bit_cast(uint32_t, om.t);
        store_curve(cv, st + LS_VOLUME_CURVE * N + v, N);
    }
    // Curve.paint's prologue for one curve of the kit.  The carried node (Curve.zig:142-148) is read at nodes[offset + cur]:
    // inside the array for every index a paint can leave (the tail, above); one that lies past it -- zh_laser_set_state only --
    // drops the carried node instead of reading outside the kit.
    __device__ __forceinline__ static void begin_curve(CurveLane &o, CurveTable &tb, const LaserArgs &a, const LkCurveDesc d, uint32_t out_len, bool nic) {
        if (!nic && o.cur < o.next && (uint64_t)d.offset + o.cur >= a.array_nodes) o.cur = o.next;
        o.begin(tb, a.sample_rate, d.function, a.nodes + d.offset, d.count, out_len, nic);
    }
    // LaserPlayer.paint's prologue (example_laser.zig:67-116), in the order the stages run
    __device__ __forceinline__ void begin(LaserTables &tb, const LaserArgs &a, uint32_t effect, float freq_mul, float carrier_mul, float modulator_mul,
                                          float modulator_rad, uint32_t out_len, bool nic) {
        dead = effect >= a.count;
        if (dead) return;
        const LkEffectDesc d = a.desc[effect];
        begin_curve(cm, tb.m, a, d.curve[LK_MODULATOR], out_len, nic);          // :78-82
        mul_m = freq_mul * modulator_mul;                                       // :83, rounded once
        om.begin(a.sample_rate, 0.0f);                                          // :86-90
        rad = modulator_rad;                                                    // :91
        begin_curve(cc, tb.c, a, d.curve[LK_CARRIER], out_len, nic);            // :94-98
        mul_c = freq_mul * carrier_mul;                                         // :99
        oc.begin(a.sample_rate, 0.0f);                                          // :102-106
        begin_curve(cv, tb.v, a, d.curve[LK_VOLUME], out_len, nic);             // :109-113
    }
    // one frame, r = its index in the sub-span.  Every `0.0f +` is a zang.zero followed by a module's `+=`: -0.0 becomes +0.0;
    // a frame a curve does not paint keeps the zero.
    __device__ __forceinline__ float frame(const LaserTables &tb, uint32_t r) {
        float x;
        const bool pm = cm.frame(tb.m, r, x);
        const float f_m = (pm ? 0.0f + x : 0.0f) * mul_m;                       // :77-83
        const float p = (0.0f + om.template frame<true>(f_m, 0.0f)) * rad;      // :85-91
        const bool pc = cc.frame(tb.c, r, x);
        const float f_c = (pc ? 0.0f + x : 0.0f) * mul_c;                       // :93-99
        const float c = 0.0f + oc.template frame<true>(f_c, p);                 // :101-106
        const bool pv = cv.frame(tb.v, r, x);
        return (pv ? 0.0f + x : 0.0f) * c;                                      // :108-115: the product; the caller adds it
    }
    __device__ __forceinline__ void end() {
        if (dead) return;
        om.end(); oc.end();                                                     // SineOsc.zig:40
    }
};

// frames [f0, f1) of one voice; s0 = the first frame of the sub-span they belong to.  `active` = false, or a dead lane, paints
// nothing; otherwise EVERY frame is added to, also where the volume curve has ended (the product is then +/-0.0, or NaN).
template <bool ZF>
__device__ __forceinline__ void laser_paint_frames(LaserLane &n, const LaserTables &tb, const Img &out, uint32_t v, uint32_t f0, uint32_t f1, uint32_t s0,
                                                   bool active) {
    const bool paints = active && !n.dead;
    frame_loop<8, ZF, 0>(out.p, v, out.stride, nullptr, nullptr, f0, f1, [&](uint32_t i, const float (&)[1], float &val) ZH_INLINE_LAMBDA {
        if (!paints) return false;
        val = n.frame(tb, i - s0);
        return true;
    });
}
#endif   // __HIPCC__
