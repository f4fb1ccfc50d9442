// hard_square.hip.h -- HardSquareInstrument (examples/modules.zig:250-289): a PulseOsc of color 0.5 times a Gate, with the
// frequency image examples/example_arpeggiator.zig:115 adds beside it (addScalarInto(span, outputs[1], params.freq)).  Two parts,
// as lead.hip.h: the state's layout as plain C++ (zh_hard_square_state <-> [word][voice] rows), and the lane (hipcc only):
// PulseOscLane of voices.hip.h on its constant-frequency path, untouched, under span_voice.hip.h's frame loop over two columns.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "span_voice.hip.h"

enum { HS_OSC_CNT = 0, kHardSquareState };   // words per voice, [word][voice]

inline void hs_pack(const zh_hard_square_state &s, uint32_t *w, size_t n, size_t v) { w[(size_t)HS_OSC_CNT * n + v] = s.osc.cnt; }
inline void hs_unpack(zh_hard_square_state &s, const uint32_t *w, size_t n, size_t v) {
    memset(&s, 0, sizeof(s));
    s.osc.cnt = w[(size_t)HS_OSC_CNT * n + v];
}
using HardSquareLayout = VoiceLayout<zh_hard_square_state, kHardSquareState, hs_pack, hs_unpack>;

#if defined(__HIPCC__)
#include "lead.hip.h"

struct HardSquarePatch {};                                             // the voice has no constants beyond color 0.5 (:281)

// The lane contract of span_voice.hip.h (load_state / store_state, begin, frame, end).  `0.0f +` is the zang.zero of :277 followed by
// PulseOsc's `+=`; where the PulseOsc paints nothing (PulseOsc.zig:82-84) temps[0] stays the zero.  The Gate adds 1.0 to a
// zeroed temp or leaves it (:283-286); zang.multiply (:287) then adds osc * gate to EVERY frame of the sub-span.
static_assert((int)ZH_HARD_SQUARE_SPAN_FREQ == LEAD_SPAN_FREQ && (int)ZH_HARD_SQUARE_SPAN_NOTE_ON == LEAD_SPAN_NOTE_ON &&
              (int)ZH_HARD_SQUARE_SPAN_FIELDS == LEAD_SPAN_FIELDS, "the leads' span fields");
struct HardSquareLane : LeadVoice<zh_hard_square_params, HardSquarePatch, 2> {
    using Layout = HardSquareLayout;
    static Args args(const zh_voice &m, const Params &p, const zh_script_span_param *sp) { return LeadVoice::args(m, p, HardSquarePatch{}, sp); }
    PulseOscLane osc;
    float freq, gate;

    __device__ __forceinline__ void load_state(const uint32_t *st, size_t N, uint32_t v) {
        osc.cnt = st[(size_t)HS_OSC_CNT * N + v];
        freq = gate = 0.0f;
        osc.begin_const(1.0f, 0.0f, 0.5f);                             // a paint without a sub-span runs no frame
    }
    __device__ __forceinline__ void store_state(uint32_t *st, size_t N, uint32_t v) const { st[(size_t)HS_OSC_CNT * N + v] = osc.cnt; }
    __device__ __forceinline__ void begin(const Args &a, const Args::Span &s, bool) {
        osc.begin_const(a.sample_rate, s.freq, 0.5f);                  // :278-282: the per-paint prologue, at every sub-span
        freq = s.freq;
        gate = s.note_on != 0 ? 1.0f : 0.0f;                              // :283-286
    }
    __device__ __forceinline__ float frame(float &f) {
        f = freq;                                                      // example_arpeggiator.zig:115
        float val = 0.0f;
        const bool painted = osc.frame_const(val);
        const float o = painted ? 0.0f + val : 0.0f;
        return o * gate;                                               // :287, gate 0 included: the product is rounded, then added
    }
    __device__ __forceinline__ void end() {}
};
#endif   // __HIPCC__
