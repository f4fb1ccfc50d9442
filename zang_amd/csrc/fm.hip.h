// fm.hip.h -- the two-operator FM voice of examples/example_fmsynth.zig as per-lane objects:
//   FMOpLane = Operator (:92-242) over Oscillator (:26-89): t, feedback1, feedback2 + an EnvLane with cubed curves
//   FMLane   = Instrument (:244-356): modulator and carrier, algorithm 0 (additive) or 1 (phase modulation)
// The reference runs every stage as its own loop through `temps`; a hand-off is an exact f32 store / load, so a register gives
// the same bits -- provided every `zero` + `+=` pair stays `0.0f + x` and no multiply-add is fused (-ffp-contract=off).
// The 22 discrete patch values (:375-398) become numbers ONCE (fm.hip k_fm_patch -> a constants table, one row per instrument);
// a paint only loads its instrument's row.  Waveform, algorithm and feedback are per lane at run time: voices with different
// patches share a launch.
// Above the lanes, as plain C++ (tests/cpp/module_state_host.cpp): the state's rows and FmLayout, zh_fm_state <-> those rows.
#pragma once
#include "module_state.hip.h"

// words of state per voice, [kFmState][n_voices]; an operator's seven, modulator first
enum { FMS_T = 0, FMS_FB1, FMS_FB2, FMS_ESTATE, FMS_ET, FMS_ELAST, FMS_ESTART, FMS_OP = 7, kFmState = 14 };
static_assert(FMS_ET == FMS_ESTATE + 1 && FMS_ELAST == FMS_ESTATE + 2 && FMS_ESTART == FMS_ESTATE + 3, "env_pack's rows");

// voice v of n: struct -> rows (w = uint32_t[kFmState * n]) and back; `reserved` is no row and reads as 0
inline void fm_pack(const zh_fm_state &st, uint32_t *w, size_t n, size_t v) {
    for (int op = 0; op < 2; op++) {
        uint32_t *s = w + (size_t)op * FMS_OP * n + v;
        const zh_fm_op_state &o = op ? st.carrier : st.modulator;
        s[(size_t)FMS_T * n] = zh_f32_bits(o.t); s[(size_t)FMS_FB1 * n] = zh_f32_bits(o.feedback1); s[(size_t)FMS_FB2 * n] = zh_f32_bits(o.feedback2);
        env_pack(o.env, s + (size_t)FMS_ESTATE * n, n);
    }
}
inline void fm_unpack(zh_fm_state &st, const uint32_t *w, size_t n, size_t v) {
    for (int op = 0; op < 2; op++) {
        const uint32_t *s = w + (size_t)op * FMS_OP * n + v;
        zh_fm_op_state &o = op ? st.carrier : st.modulator;
        o.t = zh_bits_f32(s[(size_t)FMS_T * n]); o.feedback1 = zh_bits_f32(s[(size_t)FMS_FB1 * n]); o.feedback2 = zh_bits_f32(s[(size_t)FMS_FB2 * n]);
        o.reserved = 0;
        o.env = env_unpack(s + (size_t)FMS_ESTATE * n, n);
    }
}
using FmLayout = VoiceLayout<zh_fm_state, kFmState, fm_pack, fm_unpack>;

#if defined(__HIPCC__)
#include "common.hip.h"
#include "zmath.hip.h"
#include "seq.hip.h"
#include "envelope.hip.h"
#include "span_walk.hip.h"

// rows of the constants table [kFmConsts][n_instruments]; an operator's eight, modulator first
enum { FMC_FREQ_MUL = 0, FMC_VOLUME, FMC_ATTACK, FMC_DECAY, FMC_SUSTAIN, FMC_RELEASE, FMC_TREMOLO, FMC_VIBRATO, FMC_OP = 8,
       FMC_FEEDBACK = 16,          // the modulator's feedback amount (:193-203); the carrier's is always 0 (:346)
       FMC_BITS = 17,              // algorithm | modulator waveform << 1 | carrier waveform << 3
       kFmConsts = 18 };

#ifndef ZH_FM_CHUNK
#define ZH_FM_CHUNK 4
#endif
constexpr int kFmChunk = ZH_FM_CHUNK;          // frames per chunk of fm_frame_loop

struct FMArgs {
    uint32_t *state;               // [kFmState][V]
    const float *tab;              // [kFmConsts][NI]
    uint32_t V, NI, group;
    float sample_rate;
    CImg tremolo, vibrato;         // [frame][instrument], read at the absolute frame
    F32P freq;
    BoolP note_on, nic;
};

struct FMOpLane {
    float t, fb1, fb2;                                                 // Oscillator state (:37-39)
    EnvLaneCubed env;                                                  // :230-237, .cubed throughout
    float freq_mul, volume, tremolo, vibrato, fb_amount;               // the patch's numbers
    uint32_t waveform;
    float step_freq;                                                   // params.freq * freq_mul (:209)

    __device__ __forceinline__ void load_consts(const float *tab, uint32_t NI, uint32_t j, int op, float feedback, uint32_t wave) {
        const float *c = tab + (size_t)op * FMC_OP * NI + j;
        freq_mul = c[(size_t)FMC_FREQ_MUL * NI]; volume = c[(size_t)FMC_VOLUME * NI];
        tremolo = c[(size_t)FMC_TREMOLO * NI]; vibrato = c[(size_t)FMC_VIBRATO * NI];
        env.sustain_volume = c[(size_t)FMC_SUSTAIN * NI];
        env.attack = CurveP{ZH_CURVE_CUBED, c[(size_t)FMC_ATTACK * NI]};
        env.decay = CurveP{ZH_CURVE_CUBED, c[(size_t)FMC_DECAY * NI]};
        env.release = CurveP{ZH_CURVE_CUBED, c[(size_t)FMC_RELEASE * NI]};
        fb_amount = feedback; waveform = wave;
        step_freq = 0.0f;
        env.idle(ZH_CURVE_CUBED, false);
    }
    __device__ __forceinline__ void load_state(const uint32_t *st, uint32_t V, uint32_t v, int op) {
        const uint32_t *s = st + (size_t)op * FMS_OP * V + v;
        t = zbits_f(s[(size_t)FMS_T * V]); fb1 = zbits_f(s[(size_t)FMS_FB1 * V]); fb2 = zbits_f(s[(size_t)FMS_FB2 * V]);
        env.state = s[(size_t)FMS_ESTATE * V]; env.t = zbits_f(s[(size_t)FMS_ET * V]);
        env.last_value = zbits_f(s[(size_t)FMS_ELAST * V]); env.start = zbits_f(s[(size_t)FMS_ESTART * V]);
    }
    __device__ __forceinline__ void store_state(uint32_t *st, uint32_t V, uint32_t v, int op) const {
        uint32_t *s = st + (size_t)op * FMS_OP * V + v;
        s[(size_t)FMS_T * V] = zbits_u(t); s[(size_t)FMS_FB1 * V] = zbits_u(fb1); s[(size_t)FMS_FB2 * V] = zbits_u(fb2);
        s[(size_t)FMS_ESTATE * V] = env.state; s[(size_t)FMS_ET * V] = zbits_u(env.t);
        s[(size_t)FMS_ELAST * V] = zbits_u(env.last_value); s[(size_t)FMS_ESTART * V] = zbits_u(env.start);
    }
    // the prologue of one Operator.paint: note_id_changed reaches the envelope only (:58, :230)
    __device__ __forceinline__ void begin(float sample_rate, float freq, bool note_on, bool new_note) {
        env.sample_rate = sample_rate;
        env.note_on = note_on;
        env.begin(new_note);
        step_freq = freq * freq_mul;                                   // :209, once per paint call
    }
    // One frame of Operator.paint: what `multiply(span, outputs[0], temps[0], temps[1])` adds to the output (:240).
    // ANY3 (wave-uniform): some lane of the wave has waveform 3 on an operator -- only then is the second sine evaluated.
    template <bool ANY3>
    __device__ __forceinline__ float frame(float phase, float inv_sr, float trem_in, float vib_in) {
        const float f = ((0.0f + vib_in * vibrato) + 1.0f) * step_freq;                    // temps[1] :206-209
        const float feedback = (fb1 + fb2) * fb_amount;                                    // :71
        const float p = (t + phase) * 3.14159265358979323846f * 2.0f + feedback;           // :73
        const float s = zsinf(p);                                                          // :74
        const float a = __builtin_fabsf(s);
        float sample = s;                                                                  // :75-80
        sample = waveform == 1 ? (s > 0.0f ? s : 0.0f) : sample;
        sample = waveform == 2 ? a : sample;
        if (ANY3) {
            const float s2 = zsinf(p * 2.0f);
            sample = waveform == 3 ? (s2 >= 0.0f ? a : 0.0f) : sample;
        }
        t += f * inv_sr;                                                                   // :84
        fb2 = fb1;                                                                         // :85-86
        fb1 = sample;
        const float o = ((0.0f + sample) * volume) * ((0.0f + trem_in * tremolo) + 1.0f);  // temps[0] :212-226
        const float e = env.frame_masked();                                                // temps[1] = 0 + envelope :229-237
        return o * e;
    }
    __device__ __forceinline__ void end() { t = t - truncf(t); }                           // :64; feedback1 / 2 are never reset
};

// what one frame of Instrument.paint adds: `m` to the output first (algorithm 0 only: add_m), then `c`
struct FMOut {
    float m, c;
    bool add_m;
};

struct FMLane {
    FMOpLane mod, car;
    float inv_sr;
    bool alg1;

    // the lane's patch: row j of the constants table
    __device__ __forceinline__ void load_consts(const float *tab, uint32_t NI, uint32_t j) {
        const uint32_t bits = zbits_u(tab[(size_t)FMC_BITS * NI + j]);
        alg1 = (bits & 1u) != 0;
        mod.load_consts(tab, NI, j, 0, tab[(size_t)FMC_FEEDBACK * NI + j], (bits >> 1) & 3u);
        car.load_consts(tab, NI, j, 1, 0.0f, (bits >> 3) & 3u);                            // feedback = 0 :346
        inv_sr = 0.0f;
    }
    __device__ __forceinline__ void load_state(const uint32_t *st, uint32_t V, uint32_t v) { mod.load_state(st, V, v, 0); car.load_state(st, V, v, 1); }
    __device__ __forceinline__ void store_state(uint32_t *st, uint32_t V, uint32_t v) const { mod.store_state(st, V, v, 0); car.store_state(st, V, v, 1); }
    __device__ __forceinline__ void begin(float sample_rate, float freq, bool note_on, bool new_note) {
        inv_sr = 1.0f / sample_rate;                                                       // :66
        mod.begin(sample_rate, freq, note_on, new_note);
        car.begin(sample_rate, freq, note_on, new_note);
    }
    template <bool ANY3>
    __device__ __forceinline__ void frame(float trem_in, float vib_in, FMOut &o) {
        o.m = mod.template frame<ANY3>(0.0f, inv_sr, trem_in, vib_in);                    // phase = null -> 0 (:70, :328)
        // algorithm 1: the modulator went into a zeroed temp that is the carrier's phase (:305-310); algorithm 0: phase = null
        const float ph = alg1 ? 0.0f + o.m : 0.0f;
        o.c = car.template frame<ANY3>(ph, inv_sr, trem_in, vib_in);
        o.add_m = !alg1;
    }
    __device__ __forceinline__ void end() { mod.end(); car.end(); }
};

// The frame loop of the FM kernels: seq.hip.h frame_loop's shape -- chunks of CH frames, the next chunk's loads issued before this
// one is computed, the chunk's stores after its frames -- with what frame_loop has no place for: the two LFO images are read at the
// lane's INSTRUMENT column, and with SPLIT the lane owns two output columns (2v: what the modulator adds, 2v + 1: the carrier).
//   f(trem_in, vib_in, FMOut &) -> painted
// Unsplit, a painted frame is out = (out + m) + c (algorithm 0: two rounded adds in that order, :302, :335) or out + c.
template <int CH, bool ZF, bool SPLIT, class F>
__device__ __forceinline__ void fm_frame_loop(const Img &out, uint32_t v, const CImg &trem, const CImg &vib, uint32_t j,
                                              uint32_t start, uint32_t end, F &&f) {
    constexpr int NO = SPLIT ? 2 : 1;
    const uint32_t voff = (SPLIT ? 2u * v : v) * 4u, joff = j * 4u;
    const uint32_t orow = out.stride * 4u, trow = trem.stride * 4u, vrow = vib.stride * 4u;
    const uint32_t n = end - start, nfull = n / CH;
    float oc[NO][CH], tc[CH], vc[CH];
    uint32_t i = start;
    auto load = [&](uint32_t at, float (&o)[NO][CH], float (&t)[CH], float (&x)[CH]) ZH_INLINE_LAMBDA {
        const zh_rsrc_t ro = zrow_rsrc(out.p, out.stride, at), rt = zrow_rsrc(trem.p, trem.stride, at), rv = zrow_rsrc(vib.p, vib.stride, at);
#pragma unroll
        for (int k = 0; k < CH; k++) {
            if (!ZF) {
#pragma unroll
                for (int q = 0; q < NO; q++) o[q][k] = zrow_load<1>(ro, voff + 4u * q, k * orow);
            }
            t[k] = zrow_load<1>(rt, joff, k * trow);
            x[k] = zrow_load<1>(rv, joff, k * vrow);
        }
    };
    // one frame's new column values from the old ones; returns which columns changed
    auto combine = [&](bool painted, const FMOut &r, const float (&o)[NO], float (&res)[NO]) ZH_INLINE_LAMBDA {
        if (SPLIT) {
            res[0] = (painted && r.add_m) ? o[0] + r.m : o[0];
            res[NO - 1] = painted ? o[NO - 1] + r.c : o[NO - 1];
        } else {
            const float o1 = r.add_m ? o[0] + r.m : o[0];
            res[0] = painted ? o1 + r.c : o[0];
        }
    };
    if (nfull > 0) load(i, oc, tc, vc);
    for (uint32_t c = 0; c < nfull; c++, i += CH) {
        float on[NO][CH], tn[CH], vn[CH];
        const bool more = c + 1 < nfull;
        if (more) load(i + CH, on, tn, vn);
        const zh_rsrc_t ro = zrow_rsrc(out.p, out.stride, i);
        float res[CH][NO];
        bool pm[CH], pa[CH];
#pragma unroll
        for (int k = 0; k < CH; k++) {
            FMOut r{0.0f, 0.0f, false};
            pm[k] = f(tc[k], vc[k], r);
            pa[k] = pm[k] && r.add_m;
            float o[NO];
#pragma unroll
            for (int q = 0; q < NO; q++) o[q] = ZF ? 0.0f : oc[q][k];
            combine(pm[k], r, o, res[k]);
        }
#pragma unroll
        for (int k = 0; k < CH; k++) {
            if (SPLIT) {
                if (ZF || pa[k]) zrow_store<1>(ro, voff, k * orow, res[k][0]);
                if (ZF || pm[k]) zrow_store<1>(ro, voff + 4u, k * orow, res[k][NO - 1]);
            } else if (ZF || pm[k]) zrow_store<1>(ro, voff, k * orow, res[k][0]);
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < CH; k++) {
#pragma unroll
                for (int q = 0; q < NO; q++)
                    if (!ZF) oc[q][k] = on[q][k];
                tc[k] = tn[k]; vc[k] = vn[k];
            }
        }
    }
    for (; i < end; i++) {
        const zh_rsrc_t ro = zrow_rsrc(out.p, out.stride, i);
        const float ti = zrow_load<1>(zrow_rsrc(trem.p, trem.stride, i), joff, 0), vi = zrow_load<1>(zrow_rsrc(vib.p, vib.stride, i), joff, 0);
        FMOut r{0.0f, 0.0f, false};
        const bool painted = f(ti, vi, r);
        float o[NO], res[NO];
#pragma unroll
        for (int q = 0; q < NO; q++) o[q] = ZF ? 0.0f : zrow_load<1>(ro, voff + 4u * q, 0);
        combine(painted, r, o, res);
        if (SPLIT) {
            if (ZF || (painted && r.add_m)) zrow_store<1>(ro, voff, 0, res[0]);
            if (ZF || painted) zrow_store<1>(ro, voff + 4u, 0, res[NO - 1]);
        } else if (ZF || painted) zrow_store<1>(ro, voff, 0, res[0]);
    }
}

// the frames [f0, f1) of one voice; `active` = false paints nothing (a span paint between sub-spans).  The second sine of
// waveform 3 is compiled in only where some lane of the wave needs it (any3, wave-uniform).
template <bool ZF, bool SPLIT>
__device__ __forceinline__ void fm_paint_frames(FMLane &n, const Img &out, uint32_t v, const FMArgs &a, uint32_t j, uint32_t f0, uint32_t f1,
                                                bool active, bool any3) {
    if (any3) {
        fm_frame_loop<kFmChunk, ZF, SPLIT>(out, v, a.tremolo, a.vibrato, j, f0, f1, [&](float ti, float vi, FMOut &r) ZH_INLINE_LAMBDA {
            if (!active) return false;
            n.template frame<true>(ti, vi, r);
            return true;
        });
    } else {
        fm_frame_loop<kFmChunk, ZF, SPLIT>(out, v, a.tremolo, a.vibrato, j, f0, f1, [&](float ti, float vi, FMOut &r) ZH_INLINE_LAMBDA {
            if (!active) return false;
            n.template frame<false>(ti, vi, r);
            return true;
        });
    }
}
#endif   // __HIPCC__
