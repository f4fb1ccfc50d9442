// detuned_state_host.cpp -- the detuned voice's state layout (zang_amd/csrc/detuned.hip.h DetunedLayout over ds_pack / ds_unpack: what
// zh_detuned_set_state and zh_detuned_get_state run) as a stand-alone program for AddressSanitizer + UBSan.  For n = 0, 1, 65
// and 130 voices: structs -> rows in a heap block of EXACTLY the library's size (kDetunedState * n words) -> structs again, every
// field compared on bits; and every word of every row is written exactly once, at [word][voice].
#include "../../zang_amd/csrc/detuned.hip.h"
#include "state_harness.h"

static zh_detuned_state make(uint32_t v) {
    zh_detuned_state s;
    memset(&s, 0, sizeof(s));
    for (int j = 0; j < 4; j++) s.noise.r[j] = 0x9E3779B97F4A7C15ull * (v + 1) + ((uint64_t)j << 60) + j;
    s.noise_filter.l = 0.5f + (float)v; s.noise_filter.b = -0.0f;
    s.osc.cnt = 0xFFFFFFFFu - v; s.osc.t = 0.25f * (float)v;
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = zh_bits_f32(0x7FC00001u + v); s.env.start = zh_bits_f32(0x00000001u + v);
    s.main_filter.l = -1.5f * (float)v; s.main_filter.b = zh_bits_f32(0x80000000u);
    return s;
}

int main() {
    static_assert(kDetunedState == 18, "18 words per voice");
    static_assert(sizeof(zh_detuned_state) == 104, "zh_detuned_state");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130})
        if (run<DetunedLayout>(n, make, [](const zh_detuned_state &s, const uint32_t *w, size_t n_, size_t v) {   // the scalar rows
                return w[(size_t)DS_OSC_CNT * n_ + v] == s.osc.cnt && w[(size_t)DS_ENV_STATE * n_ + v] == s.env.state &&
                       w[(size_t)DS_RNG * n_ + v] == (uint32_t)s.noise.r[0] && w[(size_t)(DS_RNG + 7) * n_ + v] == (uint32_t)(s.noise.r[3] >> 32) &&
                       w[(size_t)DS_MF_B * n_ + v] == 0x80000000u;
            })) return 1;
    // the taps are not part of the voice: packed from anything, they come back as zeros
    zh_detuned_state s = make(3), back;
    s.noise.b[2] = 7.0f; s.noise.reserved = 9;
    uint32_t w[kDetunedState];
    ds_pack(s, w, 1, 0);
    ds_unpack(back, w, 1, 0);
    if (back.noise.b[2] != 0.0f || back.noise.reserved != 0 || back.noise.r[1] != s.noise.r[1]) return fail("taps");
    printf("PASS\n");
    return 0;
}
