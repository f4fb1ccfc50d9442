// module_state.hip.h -- the state Layouts (state_block.hip.h) of the builtin modules that derive from zh_flipper: zh_<module>_state
// <-> the [word][voice] rows their kernels read (modules.hip, osc.hip, composite.hip), as plain C++, so that a stand-alone harness
// packs and reads them back under ASan and UBSan (tests/cpp/module_state_host.cpp).  The rows are in the order of the structs.
// An Envelope, a Portamento or a Curve inside a fused voice's state has the same rows from some row on: the voices' layouts
// (lead.hip.h, saw_env.hip.h, detuned.hip.h, dual.hip.h, pmctl.hip.h, laser.hip.h, curve_player.hip.h, fm.hip.h) call
// env_pack / porta_pack / curve_pack and their unpack with s = w + first_row * n + v.
#pragma once
#include "state_block.hip.h"

// ---- sub-states from a row on: s = the voice's word in the first row, rows n words apart ---------------------------------------
// Envelope: state, t, last_value, start
inline void env_pack(const zh_envelope_state &e, uint32_t *s, size_t n) {
    s[0] = e.state; s[n] = zh_f32_bits(e.t); s[2 * n] = zh_f32_bits(e.last_value); s[3 * n] = zh_f32_bits(e.start);
}
inline zh_envelope_state env_unpack(const uint32_t *s, size_t n) {
    return zh_envelope_state{s[0], zh_bits_f32(s[n]), zh_bits_f32(s[2 * n]), zh_bits_f32(s[3 * n])};
}
// Portamento: t, last_value, start
inline void porta_pack(const zh_portamento_state &p, uint32_t *s, size_t n) {
    s[0] = zh_f32_bits(p.t); s[n] = zh_f32_bits(p.last_value); s[2 * n] = zh_f32_bits(p.start);
}
inline zh_portamento_state porta_unpack(const uint32_t *s, size_t n) {
    return zh_portamento_state{zh_bits_f32(s[0]), zh_bits_f32(s[n]), zh_bits_f32(s[2 * n])};
}
// Curve: t, current_song_note, current_song_note_offset, next_song_note
inline void curve_pack(const zh_curve_module_state &c, uint32_t *s, size_t n) {
    s[0] = zh_f32_bits(c.t); s[n] = c.current_song_note; s[2 * n] = (uint32_t)c.current_song_note_offset; s[3 * n] = c.next_song_note;
}
inline zh_curve_module_state curve_unpack(const uint32_t *s, size_t n) {
    return zh_curve_module_state{zh_bits_f32(s[0]), s[n], (int32_t)s[2 * n], s[3 * n]};
}

// ---- the modules: voice v of n, struct -> rows (w = uint32_t[kWords * n]) and back ---------------------------------------------
// one word: a float phase (SineOsc, Sampler, Cycle: t) or PulseOsc's counter
template <class S> inline void t_pack(const S &s, uint32_t *w, size_t, size_t v) { w[v] = zh_f32_bits(s.t); }
template <class S> inline void t_unpack(S &s, const uint32_t *w, size_t, size_t v) { s.t = zh_bits_f32(w[v]); }
inline void pulse_pack(const zh_pulseosc_state &s, uint32_t *w, size_t, size_t v) { w[v] = s.cnt; }
inline void pulse_unpack(zh_pulseosc_state &s, const uint32_t *w, size_t, size_t v) { s.cnt = w[v]; }
using SineOscLayout = VoiceLayout<zh_sineosc_state, 1, t_pack<zh_sineosc_state>, t_unpack<zh_sineosc_state>>;
using SamplerLayout = VoiceLayout<zh_sampler_state, 1, t_pack<zh_sampler_state>, t_unpack<zh_sampler_state>>;
using CycleLayout = VoiceLayout<zh_cycle_state, 1, t_pack<zh_cycle_state>, t_unpack<zh_cycle_state>>;
using PulseOscLayout = VoiceLayout<zh_pulseosc_state, 1, pulse_pack, pulse_unpack>;

inline void envelope_pack(const zh_envelope_state &s, uint32_t *w, size_t n, size_t v) { env_pack(s, w + v, n); }
inline void envelope_unpack(zh_envelope_state &s, const uint32_t *w, size_t n, size_t v) { s = env_unpack(w + v, n); }
using EnvelopeLayout = VoiceLayout<zh_envelope_state, 4, envelope_pack, envelope_unpack>;

inline void portamento_pack(const zh_portamento_state &s, uint32_t *w, size_t n, size_t v) { porta_pack(s, w + v, n); }
inline void portamento_unpack(zh_portamento_state &s, const uint32_t *w, size_t n, size_t v) { s = porta_unpack(w + v, n); }
using PortamentoLayout = VoiceLayout<zh_portamento_state, 3, portamento_pack, portamento_unpack>;

// dval, dcount (init(): dcount = 1, Decimator.zig:14-19)
inline void decimator_pack(const zh_decimator_state &s, uint32_t *w, size_t n, size_t v) { w[v] = zh_f32_bits(s.dval); w[n + v] = zh_f32_bits(s.dcount); }
inline void decimator_unpack(zh_decimator_state &s, const uint32_t *w, size_t n, size_t v) { s = zh_decimator_state{zh_bits_f32(w[v]), zh_bits_f32(w[n + v])}; }
using DecimatorLayout = VoiceLayout<zh_decimator_state, 2, decimator_pack, decimator_unpack>;

inline void curve_module_pack(const zh_curve_module_state &s, uint32_t *w, size_t n, size_t v) { curve_pack(s, w + v, n); }
inline void curve_module_unpack(zh_curve_module_state &s, const uint32_t *w, size_t n, size_t v) { s = curve_unpack(w + v, n); }
using CurveModuleLayout = VoiceLayout<zh_curve_module_state, 4, curve_module_pack, curve_module_unpack>;

// PMOscInstrument: carrier.t, modulator.t, then the envelope (composite.hip zh_pmosc::view)
enum { PM_CARRIER_T = 0, PM_MODULATOR_T, PM_ENV, kPmoscState = PM_ENV + 4 };
inline void pmosc_pack(const zh_pmosc_state &s, uint32_t *w, size_t n, size_t v) {
    w[(size_t)PM_CARRIER_T * n + v] = zh_f32_bits(s.carrier.t); w[(size_t)PM_MODULATOR_T * n + v] = zh_f32_bits(s.modulator.t);
    env_pack(s.env, w + (size_t)PM_ENV * n + v, n);
}
inline void pmosc_unpack(zh_pmosc_state &s, const uint32_t *w, size_t n, size_t v) {
    s.carrier.t = zh_bits_f32(w[(size_t)PM_CARRIER_T * n + v]); s.modulator.t = zh_bits_f32(w[(size_t)PM_MODULATOR_T * n + v]);
    s.env = env_unpack(w + (size_t)PM_ENV * n + v, n);
}
using PmoscLayout = VoiceLayout<zh_pmosc_state, kPmoscState, pmosc_pack, pmosc_unpack>;
