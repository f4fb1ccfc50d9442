// curve_player_state_host.cpp -- the curve voice's state layout (zang_amd/csrc/curve_player.hip.h cp_pack / cp_unpack: what
// zh_curve_player_set_state and zh_curve_player_get_state run) as a stand-alone program for AddressSanitizer + UBSan.  For n = 1,
// 3 and 65 voices: structs -> rows in a heap block of EXACTLY the library's size (kCurvePlayerState * n words) -> structs again,
// every field compared on bits; every word of every row is written exactly once, at [word][voice], in the order of the struct.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zang_amd/csrc/curve_player.hip.h"

static int fail(const char *what, int a = 0, int b = 0) { printf("%s (%d, %d)\nFAIL\n", what, a, b); return 1; }

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

static int run(size_t n) {
    std::vector<zh_curve_player_state> in(n), out(n);
    for (size_t v = 0; v < n; v++) in[v] = make((uint32_t)v);
    const size_t words = (size_t)kCurvePlayerState * n;
    uint32_t *w = new uint32_t[words];                                // exactly the library's size
    for (size_t i = 0; i < words; i++) w[i] = 0xDEADBEEFu;
    for (size_t v = 0; v < n; v++) CurvePlayerLayout::pack(in[v], w, n, v);
    for (size_t i = 0; i < words; i++)
        if (w[i] == 0xDEADBEEFu) { delete[] w; return fail("a word not written", (int)(i / n), (int)(i % n)); }
    // [word][voice], the words in the struct's own order: voice v's struct is column v read top to bottom
    for (size_t v = 0; v < n; v++) {
        uint32_t col[kCurvePlayerState], want[kCurvePlayerState];
        for (int j = 0; j < kCurvePlayerState; j++) col[j] = w[(size_t)j * n + v];
        memcpy(want, &in[v], sizeof(want));
        if (memcmp(col, want, sizeof(want)) != 0) { delete[] w; return fail("row layout", (int)v); }
    }
    for (size_t v = 0; v < n; v++) CurvePlayerLayout::unpack(out[v], w, n, v);
    delete[] w;
    for (size_t v = 0; v < n; v++)
        if (memcmp(&in[v], &out[v], sizeof(zh_curve_player_state)) != 0) return fail("round trip", (int)v);
    return 0;
}

int main() {
    static_assert(kCurvePlayerState == 10 && CurvePlayerLayout::kWords == 10, "ten words per voice");
    static_assert(sizeof(zh_curve_player_state) == 40, "zh_curve_player_state: the ten words, no padding");
    static_assert(CP_CARRIER_CURVE == 0 && CP_CARRIER_T == 4 && CP_MODULATOR_CURVE == 5 && CP_MODULATOR_T == 9, "the order of example_curve.zig:41-44");
    for (size_t n : {(size_t)1, (size_t)3, (size_t)65})
        if (run(n)) return 1;
    printf("PASS\n");
    return 0;
}
