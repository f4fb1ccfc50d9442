// module_state_host.cpp -- the state layouts of the ten builtin modules whose handles share one host side (zang_amd/csrc/
// state_block.hip.h flip_get_state / flip_set_state / block_get_state / block_set_state over SineOscLayout, SamplerLayout,
// CycleLayout, PulseOscLayout, EnvelopeLayout, PortamentoLayout, DecimatorLayout, CurveModuleLayout, PmoscLayout and FmLayout: what
// zh_<module>_set_state and zh_<module>_get_state run) as a stand-alone program for AddressSanitizer + UBSan: the harness of
// lead_state_host.cpp (state_harness.h, the read-back structs prefilled with 0xA5) over the older half of the library.  For n = 0, 1, 65 and 130 voices: hostile structs -> rows in a heap
// block of EXACTLY the library's size (kWords * n words) -> structs again, compared on bits; every word of every row is written;
// and named rows hold voice v's value at column v.  The rows are named here by what the KERNELS read, not by the Layout under
// test: FMS_* (fm.hip.h FMOpLane), PM_* (composite.hip zh_pmosc::view), and for the modules of modules.hip / osc.hip, whose
// kernels take `block + k * n` as their k-th pointer (zh_envelope::f, zh_decimator::dcount, zh_portamento::f, k_curve), k itself.
#include "../../zang_amd/csrc/module_state.hip.h"
#include "../../zang_amd/csrc/fm.hip.h"
#include "state_harness.h"

static zh_envelope_state make_env(uint32_t v, uint32_t k = 0) { return zh_envelope_state{0xFFFFFFFFu - v - k, hostile(v, k), hostile(v, k + 1), hostile(v, k + 2)}; }
static zh_sineosc_state make_sine(uint32_t v) { return zh_sineosc_state{hostile(v, 0)}; }
static zh_sampler_state make_sampler(uint32_t v) { return zh_sampler_state{hostile(v, 1)}; }
static zh_cycle_state make_cycle(uint32_t v) { return zh_cycle_state{hostile(v, 2)}; }
static zh_pulseosc_state make_pulse(uint32_t v) { return zh_pulseosc_state{0xFFFFFFFFu - v}; }
static zh_envelope_state make_envelope(uint32_t v) { return make_env(v); }
static zh_portamento_state make_portamento(uint32_t v) { return zh_portamento_state{hostile(v, 3), hostile(v, 4), hostile(v, 5)}; }
static zh_decimator_state make_decimator(uint32_t v) { return zh_decimator_state{hostile(v, 0), hostile(v, 3)}; }
static zh_curve_module_state make_curve(uint32_t v) {
    return zh_curve_module_state{hostile(v, 4), 0xFFFFFFFFu - 3 * v, -(int32_t)v - 1, 0x80000000u + v};     // a negative current_song_note_offset
}
static zh_pmosc_state make_pmosc(uint32_t v) {
    zh_pmosc_state s;
    memset(&s, 0, sizeof(s));
    s.carrier.t = hostile(v, 1); s.modulator.t = hostile(v, 2); s.env = make_env(v, 3);
    return s;
}
static zh_fm_state make_fm(uint32_t v) {                              // `reserved` is no row: it reads back as 0
    zh_fm_state s;
    memset(&s, 0, sizeof(s));
    s.modulator.t = hostile(v, 0); s.modulator.feedback1 = hostile(v, 1); s.modulator.feedback2 = hostile(v, 2); s.modulator.env = make_env(v, 3);
    s.carrier.t = hostile(v, 3); s.carrier.feedback1 = hostile(v, 4); s.carrier.feedback2 = hostile(v, 5); s.carrier.env = make_env(v, 1);
    return s;
}

static bool env_rows(const zh_envelope_state &e, const uint32_t *s, size_t n) {      // s = the voice's word in the envelope's first row
    return s[0] == e.state && s[n] == zh_f32_bits(e.t) && s[2 * n] == zh_f32_bits(e.last_value) && s[3 * n] == zh_f32_bits(e.start);
}

int main() {
    // the numbers of the hand-written create / get_state / set_state these layouts replaced
    static_assert(SineOscLayout::kWords == 1 && sizeof(zh_sineosc_state) == 4, "1 word per SineOsc voice");
    static_assert(SamplerLayout::kWords == 1 && sizeof(zh_sampler_state) == 4, "1 word per Sampler voice");
    static_assert(CycleLayout::kWords == 1 && sizeof(zh_cycle_state) == 4, "1 word per Cycle voice");
    static_assert(PulseOscLayout::kWords == 1 && sizeof(zh_pulseosc_state) == 4, "1 word per PulseOsc voice");
    static_assert(EnvelopeLayout::kWords == 4 && sizeof(zh_envelope_state) == 16, "4 words per Envelope voice");
    static_assert(PortamentoLayout::kWords == 3 && sizeof(zh_portamento_state) == 12, "3 words per Portamento voice");
    static_assert(DecimatorLayout::kWords == 2 && sizeof(zh_decimator_state) == 8, "2 words per Decimator voice");
    static_assert(CurveModuleLayout::kWords == 4 && sizeof(zh_curve_module_state) == 16, "4 words per Curve voice");
    static_assert(PmoscLayout::kWords == 6 && sizeof(zh_pmosc_state) == 24, "6 words per PMOsc voice");
    static_assert(FmLayout::kWords == 14 && kFmState == 14 && sizeof(zh_fm_state) == 64, "14 words per FM voice (16 in the struct: `reserved` twice)");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130}) {
        if (run<SineOscLayout>(n, make_sine, [](const zh_sineosc_state &s, const uint32_t *w, size_t, size_t v) { return w[v] == zh_f32_bits(s.t); }, true)) return 1;
        if (run<SamplerLayout>(n, make_sampler, [](const zh_sampler_state &s, const uint32_t *w, size_t, size_t v) { return w[v] == zh_f32_bits(s.t); }, true)) return 1;
        if (run<CycleLayout>(n, make_cycle, [](const zh_cycle_state &s, const uint32_t *w, size_t, size_t v) { return w[v] == zh_f32_bits(s.t); }, true)) return 1;
        if (run<PulseOscLayout>(n, make_pulse, [](const zh_pulseosc_state &s, const uint32_t *w, size_t, size_t v) { return w[v] == s.cnt; }, true)) return 1;
        if (run<EnvelopeLayout>(n, make_envelope, [](const zh_envelope_state &s, const uint32_t *w, size_t n_, size_t v) { return env_rows(s, w + v, n_); }, true)) return 1;
        if (run<PortamentoLayout>(n, make_portamento, [](const zh_portamento_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[v] == zh_f32_bits(s.t) && w[n_ + v] == zh_f32_bits(s.last_value) && w[2 * n_ + v] == zh_f32_bits(s.start);
            }, true)) return 1;
        if (run<DecimatorLayout>(n, make_decimator, [](const zh_decimator_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[v] == zh_f32_bits(s.dval) && w[n_ + v] == zh_f32_bits(s.dcount);
            }, true)) return 1;
        if (run<CurveModuleLayout>(n, make_curve, [](const zh_curve_module_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[v] == zh_f32_bits(s.t) && w[n_ + v] == s.current_song_note && (int32_t)w[2 * n_ + v] == s.current_song_note_offset &&
                       s.current_song_note_offset < 0 && w[3 * n_ + v] == s.next_song_note;
            }, true)) return 1;
        if (run<PmoscLayout>(n, make_pmosc, [](const zh_pmosc_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)PM_CARRIER_T * n_ + v] == zh_f32_bits(s.carrier.t) && w[(size_t)PM_MODULATOR_T * n_ + v] == zh_f32_bits(s.modulator.t) &&
                       env_rows(s.env, w + (size_t)PM_ENV * n_ + v, n_);
            }, true)) return 1;
        if (run<FmLayout>(n, make_fm, [](const zh_fm_state &s, const uint32_t *w, size_t n_, size_t v) {
                for (int op = 0; op < 2; op++) {
                    const zh_fm_op_state &o = op ? s.carrier : s.modulator;
                    const uint32_t *r = w + (size_t)op * FMS_OP * n_ + v;
                    if (r[(size_t)FMS_T * n_] != zh_f32_bits(o.t) || r[(size_t)FMS_FB1 * n_] != zh_f32_bits(o.feedback1) || r[(size_t)FMS_FB2 * n_] != zh_f32_bits(o.feedback2) ||
                        r[(size_t)FMS_ESTATE * n_] != o.env.state || r[(size_t)FMS_ET * n_] != zh_f32_bits(o.env.t) ||
                        r[(size_t)FMS_ELAST * n_] != zh_f32_bits(o.env.last_value) || r[(size_t)FMS_ESTART * n_] != zh_f32_bits(o.env.start)) return false;
                }
                return true;
            }, true)) return 1;
    }
    printf("PASS\n");
    return 0;
}
