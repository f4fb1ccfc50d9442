// pmctl_state_host.cpp -- the state layout of the controlled phase-modulation voice (zang_amd/csrc/pmctl.hip.h PmctlLayout: what
// zh_pmctl_set_state and zh_pmctl_get_state run through span_voice.hip.h's voice_get_state / voice_set_state) as a stand-alone
// program for AddressSanitizer + UBSan, as lead_state_host.cpp and dual_state_host.cpp run the other layouts.  For n = 0, 1, 65 and
// 130 voices: structs -> rows in a heap block of EXACTLY the library's size (kWords * n words) -> structs again, every field
// compared on bits; and every word of every row is written exactly once, at [word][voice].
#include "../../zang_amd/csrc/pmctl.hip.h"
#include "state_harness.h"

static zh_pmctl_state make(uint32_t v) {
    zh_pmctl_state s;
    memset(&s, 0, sizeof(s));
    s.ratio.t = 1.0f / (float)(v + 2); s.ratio.last_value = zh_bits_f32(0x7FC00011u + v); s.ratio.start = zh_bits_f32(0x80000000u);
    s.multiplier.t = 1.0f / (float)(v + 3); s.multiplier.last_value = zh_bits_f32(0x00000101u + v); s.multiplier.start = -(float)v;
    s.carrier.t = (float)v + 0.25f; s.modulator.t = zh_bits_f32(0xFF800000u);
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = zh_bits_f32(0x7FC00001u + v); s.env.start = zh_bits_f32(0x00000001u + v);
    return s;
}

// the words of one voice in the order of the rows
static void words_of(const zh_pmctl_state &s, uint32_t (&w)[kPmctlState]) {
    const uint32_t x[kPmctlState] = {zh_f32_bits(s.ratio.t), zh_f32_bits(s.ratio.last_value), zh_f32_bits(s.ratio.start),
                                     zh_f32_bits(s.multiplier.t), zh_f32_bits(s.multiplier.last_value), zh_f32_bits(s.multiplier.start),
                                     zh_f32_bits(s.carrier.t), zh_f32_bits(s.modulator.t),
                                     s.env.state, zh_f32_bits(s.env.t), zh_f32_bits(s.env.last_value), zh_f32_bits(s.env.start)};
    memcpy(w, x, sizeof(x));
}

int main() {
    static_assert(kPmctlState == 12 && sizeof(zh_pmctl_state) == 48, "12 words per controlled voice");
    static_assert(PC_RATIO_T == 0 && PC_MULT_T == 3 && PC_CARRIER_T == 6 && PC_MODULATOR_T == 7 && PC_ENV_STATE == 8 && PC_ENV_START == 11,
                  "the rows follow the struct's fields");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130})
        if (run<PmctlLayout>(n, make, [](const zh_pmctl_state &s, const uint32_t *w, size_t n_, size_t v) {   // row k holds voice v's word k at column v
                uint32_t want[kPmctlState];
                words_of(s, want);
                for (size_t k = 0; k < (size_t)kPmctlState; k++)
                    if (w[k * n_ + v] != want[k]) return false;
                return true;
            })) return 1;
    printf("PASS\n");
    return 0;
}
