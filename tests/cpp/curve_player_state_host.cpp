// curve_player_state_host.cpp -- the curve voice's state layout (zang_amd/csrc/curve_player.hip.h cp_pack / cp_unpack: what
// zh_curve_player_set_state and zh_curve_player_get_state run) as a stand-alone program for AddressSanitizer + UBSan.  For n = 1,
// 3 and 65 voices: structs -> rows in a heap block of EXACTLY the library's size (kCurvePlayerState * n words) -> structs again,
// every field compared on bits; every word of every row is written exactly once, at [word][voice], in the order of the struct.
#include "../../zang_amd/csrc/curve_player.hip.h"
#include "state_harness.h"

static zh_curve_module_state curve(uint32_t v, uint32_t salt) {
    return zh_curve_module_state{zh_bits_f32(0x7FC00001u + v + salt), 0xFFFFFFFFu - v - salt, -(int32_t)(v + salt) - 1, 0x80000000u + v * 3 + salt};
}
static zh_curve_player_state make(uint32_t v) {
    zh_curve_player_state s;
    memset(&s, 0, sizeof(s));
    s.carrier_curve = curve(v, 10);
    s.carrier.t = zh_bits_f32(0x80000000u);                           // -0.0
    s.modulator_curve = curve(v, 20);
    s.modulator.t = 0.25f * (float)v + 0.125f;
    return s;
}

int main() {
    static_assert(kCurvePlayerState == 10 && CurvePlayerLayout::kWords == 10, "ten words per voice");
    static_assert(sizeof(zh_curve_player_state) == 40, "zh_curve_player_state: the ten words, no padding");
    static_assert(CP_CARRIER_CURVE == 0 && CP_CARRIER_T == 4 && CP_MODULATOR_CURVE == 5 && CP_MODULATOR_T == 9, "the order of example_curve.zig:41-44");
    for (size_t n : {(size_t)1, (size_t)3, (size_t)65})
        if (run<CurvePlayerLayout>(n, make, [](const zh_curve_player_state &s, const uint32_t *w, size_t n_, size_t v) {
                // the words in the struct's own order: voice v's struct is column v read top to bottom
                uint32_t col[kCurvePlayerState], want[kCurvePlayerState];
                for (int j = 0; j < kCurvePlayerState; j++) col[j] = w[(size_t)j * n_ + v];
                memcpy(want, &s, sizeof(want));
                return memcmp(col, want, sizeof(want)) == 0;
            })) return 1;
    printf("PASS\n");
    return 0;
}
