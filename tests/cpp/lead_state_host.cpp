// lead_state_host.cpp -- the state layouts of the six voices whose handles share one host side (zang_amd/csrc/span_voice.hip.h
// voice_get_state / voice_set_state over PortaLayout, VibratoLayout, HardSquareLayout, SawEnvLayout, DetunedLayout, LaserLayout: what
// zh_<voice>_set_state and zh_<voice>_get_state run) as a stand-alone program for AddressSanitizer + UBSan.  For n = 0, 1, 65 and
// 130 voices: structs -> rows in a heap block of EXACTLY the library's size (kWords * n words) -> structs again, every field
// compared on bits; and every word of every row is written exactly once, at [word][voice].
#include "../../zang_amd/csrc/lead.hip.h"
#include "../../zang_amd/csrc/hard_square.hip.h"
#include "../../zang_amd/csrc/saw_env.hip.h"
#include "../../zang_amd/csrc/detuned.hip.h"
#include "../../zang_amd/csrc/laser.hip.h"
#include "state_harness.h"

static zh_porta_state make_porta(uint32_t v) {
    zh_porta_state s;
    memset(&s, 0, sizeof(s));
    s.porta.t = 1.0f / (float)(v + 2); s.porta.last_value = 220.0f + (float)v; s.porta.start = zh_bits_f32(0x80000000u);
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = zh_bits_f32(0x7FC00001u + v); s.env.start = zh_bits_f32(0x00000001u + v);
    s.osc.t = 0.25f * (float)v;
    s.prev_note_on = v & 1;
    return s;
}
static zh_vibrato_state make_vibrato(uint32_t v) {
    zh_vibrato_state s;
    memset(&s, 0, sizeof(s));
    s.vib.t = zh_bits_f32(0x7FC00001u + v);
    s.osc.cnt = 0xFFFFFFFFu - v;
    return s;
}
static zh_hard_square_state make_hard_square(uint32_t v) {
    zh_hard_square_state s;
    memset(&s, 0, sizeof(s));
    s.osc.cnt = 0x80000000u + v;
    return s;
}
static zh_saw_env_state make_saw_env(uint32_t v) {
    zh_saw_env_state s;
    memset(&s, 0, sizeof(s));
    s.osc.cnt = 0xFFFFFFFFu - v; s.osc.t = zh_bits_f32(0x80000000u);
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = zh_bits_f32(0x7FC00001u + v); s.env.start = zh_bits_f32(0x00000001u + v);
    return s;
}
static zh_detuned_state make_detuned(uint32_t v) {                    // the taps of zh_noise_state are not part of the voice: zero
    zh_detuned_state s;
    memset(&s, 0, sizeof(s));
    for (int j = 0; j < 4; j++) s.noise.r[j] = 0x9E3779B97F4A7C15ull * (v + 1) + ((uint64_t)j << 60) + j;
    s.noise_filter.l = 0.5f + (float)v; s.noise_filter.b = -0.0f;
    s.osc.cnt = 0xFFFFFFFFu - v; s.osc.t = 0.25f * (float)v;
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = zh_bits_f32(0x7FC00001u + v); s.env.start = zh_bits_f32(0x00000001u + v);
    s.main_filter.l = -1.5f * (float)v; s.main_filter.b = zh_bits_f32(0x80000000u);
    return s;
}
static zh_curve_module_state make_curve(uint32_t v, uint32_t k) {
    return zh_curve_module_state{zh_bits_f32(0x7FC00001u + 3 * v + k), 10 * v + k, -(int32_t)(v + k) - 1, 0xFFFFFFFFu - v - k};
}
static zh_laser_state make_laser(uint32_t v) {
    zh_laser_state s;
    memset(&s, 0, sizeof(s));
    s.carrier_curve = make_curve(v, 0); s.carrier.t = 0.25f * (float)v;
    s.modulator_curve = make_curve(v, 1); s.modulator.t = zh_bits_f32(0x80000000u);
    s.volume_curve = make_curve(v, 2);
    return s;
}

int main() {
    static_assert(kPortaState == 9, "9 words per portamento voice");
    static_assert(kVibratoState == 2, "2 words per vibrato voice");
    static_assert(sizeof(zh_porta_state) == 36, "zh_porta_state");
    static_assert(sizeof(zh_vibrato_state) == 8, "zh_vibrato_state");
    static_assert(kHardSquareState == 1 && sizeof(zh_hard_square_state) == 4, "1 word per HardSquare voice");
    static_assert(kSawEnvState == 6 && sizeof(zh_saw_env_state) == 24, "6 words per SawEnv voice");
    static_assert(kDetunedState == 18 && sizeof(zh_detuned_state) == 104, "18 words per detuned voice");
    static_assert(kLaserState == 14 && sizeof(zh_laser_state) == 56, "14 words per laser voice");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130}) {
        if (run<PortaLayout>(n, make_porta, [](const zh_porta_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)PS_ENV_STATE * n_ + v] == s.env.state && w[(size_t)PS_PREV_NOTE_ON * n_ + v] == s.prev_note_on &&
                       w[(size_t)PS_PORTA_START * n_ + v] == 0x80000000u && w[(size_t)PS_OSC_T * n_ + v] == zh_f32_bits(s.osc.t) &&
                       w[(size_t)PS_PORTA_T * n_ + v] == zh_f32_bits(s.porta.t);
            })) return 1;
        if (run<VibratoLayout>(n, make_vibrato, [](const zh_vibrato_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)VS_OSC_CNT * n_ + v] == s.osc.cnt && w[(size_t)VS_VIB_T * n_ + v] == zh_f32_bits(s.vib.t);
            })) return 1;
        if (run<HardSquareLayout>(n, make_hard_square, [](const zh_hard_square_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)HS_OSC_CNT * n_ + v] == s.osc.cnt;
            })) return 1;
        if (run<SawEnvLayout>(n, make_saw_env, [](const zh_saw_env_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)SE_OSC_CNT * n_ + v] == s.osc.cnt && w[(size_t)SE_OSC_T * n_ + v] == 0x80000000u &&
                       w[(size_t)SE_ENV_STATE * n_ + v] == s.env.state && w[(size_t)SE_ENV_START * n_ + v] == zh_f32_bits(s.env.start);
            })) return 1;
        if (run<DetunedLayout>(n, make_detuned, [](const zh_detuned_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)DS_OSC_CNT * n_ + v] == s.osc.cnt && w[(size_t)DS_ENV_STATE * n_ + v] == s.env.state &&
                       w[(size_t)DS_RNG * n_ + v] == (uint32_t)s.noise.r[0] && w[(size_t)(DS_RNG + 7) * n_ + v] == (uint32_t)(s.noise.r[3] >> 32) &&
                       w[(size_t)DS_MF_B * n_ + v] == 0x80000000u;
            })) return 1;
        if (run<LaserLayout>(n, make_laser, [](const zh_laser_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)LS_CARRIER_CURVE * n_ + v] == zh_f32_bits(s.carrier_curve.t) && w[(size_t)LS_CARRIER_T * n_ + v] == zh_f32_bits(s.carrier.t) &&
                       w[(size_t)(LS_MODULATOR_CURVE + 2) * n_ + v] == (uint32_t)s.modulator_curve.current_song_note_offset &&
                       w[(size_t)LS_MODULATOR_T * n_ + v] == 0x80000000u && w[(size_t)(LS_VOLUME_CURVE + 3) * n_ + v] == s.volume_curve.next_song_note;
            })) return 1;
    }
    printf("PASS\n");
    return 0;
}
