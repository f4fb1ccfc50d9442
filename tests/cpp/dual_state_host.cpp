// dual_state_host.cpp -- the state layout of the two-source voice (zang_amd/csrc/dual.hip.h DualLayout: what zh_dual_set_state and
// zh_dual_get_state run through span_voice.hip.h's voice_get_state / voice_set_state) as a stand-alone program for AddressSanitizer
// + UBSan: the harness of lead_state_host.cpp, which runs the other six layouts, over the seventh.  For n = 0, 1, 65 and 130
// voices: structs -> rows in a heap block of EXACTLY the library's size (kWords * n words) -> structs again, every field compared
// on bits; and every word of every row is written exactly once, at [word][voice].
#include "../../zang_amd/csrc/dual.hip.h"
#include "state_harness.h"

static zh_dual_state make_dual(uint32_t v) {
    zh_dual_state s;
    memset(&s, 0, sizeof(s));
    s.osc.cnt = 0xFFFFFFFFu - v; s.osc.t = zh_bits_f32(0x80000000u);
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = zh_bits_f32(0x7FC00001u + v); s.env.start = zh_bits_f32(0x00000001u + v);
    return s;
}

int main() {
    static_assert(kDualState == 6 && sizeof(zh_dual_state) == 24, "6 words per two-source voice");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130}) {
        if (run<DualLayout>(n, make_dual, [](const zh_dual_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)DL_OSC_CNT * n_ + v] == s.osc.cnt && w[(size_t)DL_OSC_T * n_ + v] == 0x80000000u &&
                       w[(size_t)DL_ENV_STATE * n_ + v] == s.env.state && w[(size_t)DL_ENV_T * n_ + v] == zh_f32_bits(s.env.t) &&
                       w[(size_t)DL_ENV_LAST * n_ + v] == zh_f32_bits(s.env.last_value) && w[(size_t)DL_ENV_START * n_ + v] == zh_f32_bits(s.env.start);
            })) return 1;
    }
    printf("PASS\n");
    return 0;
}
