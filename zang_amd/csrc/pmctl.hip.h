// pmctl.hip.h -- the controlled phase-modulation voice of examples/example_mouse.zig: PMOscInstrument (:24-73) over
// PhaseModOscillator (examples/modules.zig:6-77) with `relative` a parameter and ratio and multiplier SIGNALS, and MainModule.paint
// (:148-211), where each of the two signals is a Portamento driven by its own impulse stream.  Three parts:
//   the state's layout as plain C++ (zh_pmctl_state <-> [word][voice] rows; tests/cpp/pmctl_state_host.cpp);
//   the three-cursor walk as plain C++ (pmctl_walk: three independently scheduled row lists -> segments; the kernels and
//   tests/cpp/pmctl_walk_host.cpp run the same text);
//   the lane and its frame loop (hipcc only): PortamentoLane and SineOscLane of voices.hip.h and EnvLaneCubed of envelope.hip.h,
//   untouched, in the reference's stage order.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"
#include "module_state.hip.h"

// ---- the state's layout ------------------------------------------------------------------------------------------------
// words per voice, [word][voice], in the order of the struct
enum { PC_RATIO_T = 0, PC_RATIO_LAST, PC_RATIO_START, PC_MULT_T, PC_MULT_LAST, PC_MULT_START, PC_CARRIER_T, PC_MODULATOR_T,
       PC_ENV_STATE, PC_ENV_T, PC_ENV_LAST, PC_ENV_START, kPmctlState };

inline void pc_pack(const zh_pmctl_state &s, uint32_t *w, size_t n, size_t v) {
    porta_pack(s.ratio, w + (size_t)PC_RATIO_T * n + v, n);
    porta_pack(s.multiplier, w + (size_t)PC_MULT_T * n + v, n);
    w[(size_t)PC_CARRIER_T * n + v] = zh_f32_bits(s.carrier.t); w[(size_t)PC_MODULATOR_T * n + v] = zh_f32_bits(s.modulator.t);
    env_pack(s.env, w + (size_t)PC_ENV_STATE * n + v, n);
}
inline void pc_unpack(zh_pmctl_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.ratio = porta_unpack(w + (size_t)PC_RATIO_T * n + v, n);
    s.multiplier = porta_unpack(w + (size_t)PC_MULT_T * n + v, n);
    s.carrier.t = zh_bits_f32(w[(size_t)PC_CARRIER_T * n + v]); s.modulator.t = zh_bits_f32(w[(size_t)PC_MODULATOR_T * n + v]);
    s.env = env_unpack(w + (size_t)PC_ENV_STATE * n + v, n);
}
using PmctlLayout = VoiceLayout<zh_pmctl_state, kPmctlState, pc_pack, pc_unpack>;

// ---- the three-cursor walk ---------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#define PMCTL_HD __host__ __device__ __forceinline__
#define PMCTL_LAMBDA __attribute__((always_inline))    // as ZH_INLINE_LAMBDA: an outlined closure forces the lane out of VGPRs
#else
#define PMCTL_HD inline
#define PMCTL_LAMBDA
#endif

enum { PMCTL_NOTES = 0, PMCTL_RATIO, PMCTL_MULT, kPmctlStreams };      // bit s of a segment's mask = stream s is inside a sub-span

// a [span][voice] table as the walk reads it (zh_script_span_table); anything with these members and operator[] will do
struct PmctlTable {
    uint32_t K;
    const uint32_t *count, *start, *end;
    const uint8_t *nic;
};
// a stream without rows: the controls of the plain paints
struct PmctlNoTable {
    struct Zero { PMCTL_HD uint32_t operator[](size_t) const { return 0; } };
    uint32_t K;
    Zero count, start, end, nic;
};

// One stream's cursor: span_walk.hip.h's per-lane walk, so that a stream here is cut exactly as a span paint of its own table
// would cut it -- the first min(count[v], K) rows; a row begins at its first frame and ends after its last; a row that starts
// before the previous one ends, or outside the buffer, is never reached and ends THIS stream's list; one that ends before it
// starts, or after the buffer, runs to the buffer end without its epilogue.
struct PmctlCursor {
    uint32_t cnt, k, cur_end, next_start;
    bool active;
    template <class TB> PMCTL_HD void init(const TB &tb, size_t v, bool live) {
        const uint32_t c = live ? (uint32_t)tb.count[v] : 0u;
        cnt = c < tb.K ? c : tb.K;
        k = 0; cur_end = 0; active = false;
        next_start = cnt > 0 ? (uint32_t)tb.start[v] : 0xffffffffu;
    }
    // the rows that end / begin at frame i
    template <class TB, class Begin, class End> PMCTL_HD void advance(const TB &tb, size_t V, size_t v, uint32_t i, Begin &&begin, End &&end_fn) {
        for (;;) {
            if (active) {
                if (i == cur_end) {
                    end_fn(); active = false; k++;
                    next_start = k < cnt ? (uint32_t)tb.start[(size_t)k * V + v] : 0xffffffffu;
                    continue;
                }
                break;
            }
            if (i == next_start) {
                const size_t idx = (size_t)k * V + v;
                cur_end = tb.end[idx];
                begin(idx, tb.nic[idx] != 0);
                active = true;
                continue;
            }
            break;
        }
    }
    // this stream's next boundary after frame i, buf_end where there is none (unsorted / out-of-range entries never fire)
    PMCTL_HD uint32_t next(uint32_t i, uint32_t buf_end) const {
        const uint32_t ev = active ? cur_end : next_start;
        return (ev > i && ev < buf_end) ? ev : buf_end;
    }
};

// Voice v of V over [buf_start, buf_end): the buffer as segments that end at the nearest next boundary of ANY of the three
// streams (and, on the device, of any lane of the wave: `wave_min` is the wave-wide minimum, the identity on the host).
//   begin(s, kv, nic)          row kv of stream s starts      end_fn(s)   it ended
//   segment(f0, f1, mask)      frames [f0, f1); bit s of mask = stream s is inside a row there
// The three streams keep independent state (a Portamento each, and the voice), and at one frame every stream's ends and begins
// are handled before any frame is painted: the order in which coinciding boundaries of DIFFERENT streams are handled cannot
// show in the output.  It is notes, ratio, multiplier here.
template <class TN, class TR, class TM, class Min, class Begin, class Segment, class End>
PMCTL_HD void pmctl_walk(const TN &tn, const TR &tr, const TM &tm, size_t V, size_t v, bool live, uint32_t buf_start, uint32_t buf_end,
                         Min &&wave_min, Begin &&begin, Segment &&segment, End &&end_fn) {
    PmctlCursor cn, cr, cm;
    cn.init(tn, v, live); cr.init(tr, v, live); cm.init(tm, v, live);
    auto advance = [&](uint32_t i) PMCTL_LAMBDA {
        cn.advance(tn, V, v, i, [&](size_t kv, bool nic) PMCTL_LAMBDA { begin((int)PMCTL_NOTES, kv, nic); }, [&]() PMCTL_LAMBDA { end_fn((int)PMCTL_NOTES); });
        cr.advance(tr, V, v, i, [&](size_t kv, bool nic) PMCTL_LAMBDA { begin((int)PMCTL_RATIO, kv, nic); }, [&]() PMCTL_LAMBDA { end_fn((int)PMCTL_RATIO); });
        cm.advance(tm, V, v, i, [&](size_t kv, bool nic) PMCTL_LAMBDA { begin((int)PMCTL_MULT, kv, nic); }, [&]() PMCTL_LAMBDA { end_fn((int)PMCTL_MULT); });
    };
    uint32_t i = buf_start;
    while (i < buf_end) {
        advance(i);
        uint32_t ev = cn.next(i, buf_end);
        const uint32_t er = cr.next(i, buf_end), em = cm.next(i, buf_end);
        ev = er < ev ? er : ev;
        ev = em < ev ? em : ev;
        const uint32_t seg_end = wave_min(ev);
        segment(i, seg_end, (cn.active ? 1u << PMCTL_NOTES : 0u) | (cr.active ? 1u << PMCTL_RATIO : 0u) | (cm.active ? 1u << PMCTL_MULT : 0u));
        i = seg_end;
    }
    advance(buf_end);                                                  // rows that end with the buffer; empty rows at buf_end
}

// ---- the lane --------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "common.hip.h"
#include "zmath.hip.h"
#include "seq.hip.h"
#include "envelope.hip.h"
#include "voices.hip.h"

// one control of zh_pmctl_paint_controlled as the kernel reads it
struct PmctlCtlP {
    const float *value;                                               // [span][voice]
    const uint32_t *note_on;
    F32P scale;
};
struct PmctlArgs {
    uint32_t V;
    uint32_t *state;                                                  // [kPmctlState][V]
    float sample_rate;
    zh_pmctl_patch patch;
    F32P freq;
    BoolP note_on, relative;
    const float *sf;                                                  // the notes' span arrays (ZH_PMCTL_SPAN_*), or NULL
    const uint32_t *sn;
    CobP ratio, mult;                                                 // paint / paint_spans
    PmctlCtlP rc, mc;                                                 // paint_controlled
    Img stale;                                                        // temps[1], the carried envelope image; p = NULL: none
};

// `0.0f +` is a zang.zero followed by a module's `+=`: -0.0 becomes +0.0.  No product is contracted with an add.
struct PmctlLane {
    PortamentoLane pr, pm;                                            // the ratio's and the multiplier's Portamento
    SineOscLane car, mod;
    EnvLaneCubed env;                                                 // all three curves are cubed (example_mouse.zig:65-67)
    float freq;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        const uint32_t *s = st + v;
        pr.t = zbits_f(s[(size_t)PC_RATIO_T * N]); pr.last = zbits_f(s[(size_t)PC_RATIO_LAST * N]); pr.st = zbits_f(s[(size_t)PC_RATIO_START * N]);
        pm.t = zbits_f(s[(size_t)PC_MULT_T * N]); pm.last = zbits_f(s[(size_t)PC_MULT_LAST * N]); pm.st = zbits_f(s[(size_t)PC_MULT_START * N]);
        car.t = zbits_f(s[(size_t)PC_CARRIER_T * N]); mod.t = zbits_f(s[(size_t)PC_MODULATOR_T * N]);
        env.state = s[(size_t)PC_ENV_STATE * N]; env.t = zbits_f(s[(size_t)PC_ENV_T * N]);
        env.last_value = zbits_f(s[(size_t)PC_ENV_LAST * N]); env.start = zbits_f(s[(size_t)PC_ENV_START * N]);
        // a paint without a sub-span runs no frame; the fields the prologues set are given values all the same
        freq = 0.0f;
        pr.goal = pr.t_step = 0.0f; pr.tag = ZH_CURVE_INSTANTANEOUS; pr.flat = true;
        pm.goal = pm.t_step = 0.0f; pm.tag = ZH_CURVE_INSTANTANEOUS; pm.flat = true;
        car.t_step = car.inv_sr = mod.t_step = mod.inv_sr = 0.0f;
        env.idle(ZH_CURVE_CUBED);
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const {
        uint32_t *s = st + v;
        s[(size_t)PC_RATIO_T * N] = zbits_u(pr.t); s[(size_t)PC_RATIO_LAST * N] = zbits_u(pr.last); s[(size_t)PC_RATIO_START * N] = zbits_u(pr.st);
        s[(size_t)PC_MULT_T * N] = zbits_u(pm.t); s[(size_t)PC_MULT_LAST * N] = zbits_u(pm.last); s[(size_t)PC_MULT_START * N] = zbits_u(pm.st);
        s[(size_t)PC_CARRIER_T * N] = zbits_u(car.t); s[(size_t)PC_MODULATOR_T * N] = zbits_u(mod.t);
        s[(size_t)PC_ENV_STATE * N] = env.state; s[(size_t)PC_ENV_T * N] = zbits_u(env.t);
        s[(size_t)PC_ENV_LAST * N] = zbits_u(env.last_value); s[(size_t)PC_ENV_START * N] = zbits_u(env.start);
    }
    // the prologues of PMOscInstrument.paint's three modules (example_mouse.zig:55-70), at every note sub-span
    __device__ __forceinline__ void begin_note(const PmctlArgs &a, float freq_, bool note_on, bool nic) {
        const zh_pmctl_patch &p = a.patch;
        freq = freq_;
        mod.begin(a.sample_rate, 0.0f);                                // modules.zig:59-63: the frequency-buffer path
        car.begin(a.sample_rate, freq_);                               // :70-74: a constant frequency
        env.sample_rate = a.sample_rate;                               // example_mouse.zig:63-70
        env.sustain_volume = p.sustain_volume;
        env.attack = CurveP{ZH_CURVE_CUBED, p.attack};
        env.decay = CurveP{ZH_CURVE_CUBED, p.decay};
        env.release = CurveP{ZH_CURVE_CUBED, p.release};
        env.note_on = note_on;
        env.begin(nic);
    }
    __device__ __forceinline__ void end_note() { car.end(); mod.end(); }   // SineOsc.zig:40, both oscillators
    // a control's Portamento.paint prologue (example_mouse.zig:153-168 / :177-189) at one of ITS sub-spans
    __device__ __forceinline__ void begin_ctl(PortamentoLane &p, const PmctlArgs &a, const PmctlCtlP &c, size_t kv, float scale, bool nic) {
        p.begin(a.sample_rate, a.patch.ctl_curve, a.patch.ctl_glide, c.value[kv] * scale, c.note_on[kv] != 0, true, nic);
    }
    // One frame inside a note sub-span: r, m = ratio and multiplier at the frame; RB = the ratio is a buffer; s = the stale temp
    // (zang_hip.h); -> what is added to outputs[0], e = the envelope's temp.
    __device__ __forceinline__ float frame(float r, float m, bool rb, bool rel, float s, float &e) {
        const float mf = rel ? (rb ? s + r * freq : freq * r) : r;     // modules.zig:42-57
        const float mo = 0.0f + mod.template frame<true>(mf, 0.0f);    // :58-63
        const float ph = 0.0f + mo * m;                                // :64-68
        const float c = 0.0f + car.template frame<false>(0.0f, ph);    // :69-74
        const float o = 0.0f + c;                                      // :75
        e = env.frame_masked();                                        // example_mouse.zig:62-70
        return o * e;                                                  // :71 (the product is rounded, then added)
    }
};

// Every voice's paint: the walk over the notes' table TN and, CTL, the two controls' tables, one lane per voice (kSeqBlock-lane
// blocks over seq_grid(V)).  Idle lanes of the last wave shadow voice 0 read-only and store nothing.  The state words are loaded
// and stored once; the output goes through frame_loop; the ratio, multiplier and stale images are read by the lane itself at
// the absolute frame.  Wave-uniform choices (a cob's tag, the stale image) are run-time branches.
template <bool ZF, bool CTL, class TN, class TR, class TM>
__device__ __forceinline__ void pmctl_voice(const PmctlArgs &a, const TN &tn, const TR &tr, const TM &tm, const Img &out, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    PmctlLane n;
    n.load_state(a.state, a.V, v);
    const float freq_d = a.freq.get(v);
    const bool on_d = a.note_on.get(v), rel = a.relative.get(v);
    const float rconst = a.ratio.c.get(v), mconst = a.mult.c.get(v);
    const float rscale = a.rc.scale.get(v), mscale = a.mc.scale.get(v);
    const bool rb = CTL || a.ratio.is_buffer != 0, mb = CTL || a.mult.is_buffer != 0;
    const float *rimg = a.ratio.b.p, *mimg = a.mult.b.p;
    const size_t rstr = a.ratio.b.stride, mstr = a.mult.b.stride;
    float *simg = a.stale.p;
    const size_t sstr = a.stale.stride;
    const float *const *no_in = nullptr;
    pmctl_walk(tn, tr, tm, a.V, v, live, start, end,
               [&](uint32_t ev) ZH_INLINE_LAMBDA {
#pragma unroll
                   for (int off = 32; off > 0; off >>= 1) ev = min(ev, (uint32_t)__shfl_xor((int)ev, off));
                   return (uint32_t)__builtin_amdgcn_readfirstlane(ev);
               },
               [&](int s, size_t kv, bool nic) ZH_INLINE_LAMBDA {
                   if (s == PMCTL_NOTES) n.begin_note(a, span_f(a.sf, kv, freq_d), span_u(a.sn, kv, on_d ? 1u : 0u) != 0, nic);
                   else if (s == PMCTL_RATIO) n.begin_ctl(n.pr, a, a.rc, kv, rscale, nic);
                   else n.begin_ctl(n.pm, a, a.mc, kv, mscale, nic);
               },
               [&](uint32_t f0, uint32_t f1, uint32_t mask) ZH_INLINE_LAMBDA {
                   if (!live) return;
                   const bool note = (mask & (1u << PMCTL_NOTES)) != 0;
                   const bool ra = (mask & (1u << PMCTL_RATIO)) != 0, ma = (mask & (1u << PMCTL_MULT)) != 0;
                   frame_loop<8, ZF, 0>(out.p, v, out.stride, no_in, nullptr, f0, f1, [&](uint32_t i, const float (&)[1], float &val) ZH_INLINE_LAMBDA {
                       float r = rconst, m = mconst;
                       if constexpr (CTL) {                            // the controls move whether or not a note sounds
                           r = 0.0f; m = 0.0f;                         // example_mouse.zig:149, :172: outside every sub-span the zero
                           if (ra) r = 0.0f + n.pr.frame();
                           if (ma) m = 0.0f + n.pm.frame();
                       }
                       if (!note) return false;
                       if constexpr (!CTL) {
                           if (rb) r = rimg[(size_t)i * rstr + v];
                           if (mb) m = mimg[(size_t)i * mstr + v];
                       }
                       float s = 0.0f, e;
                       if (simg && rb && rel) s = simg[(size_t)i * sstr + v];
                       val = n.frame(r, m, rb, rel, s, e);
                       if (simg) simg[(size_t)i * sstr + v] = e;
                       return true;
                   });
               },
               [&](int s) ZH_INLINE_LAMBDA { if (s == PMCTL_NOTES) n.end_note(); });
    if (live) n.store_state(a.state, a.V, v);
}
#endif   // __HIPCC__
