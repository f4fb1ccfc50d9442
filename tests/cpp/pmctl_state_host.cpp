// pmctl_state_host.cpp -- the state layout of the controlled phase-modulation voice (zang_amd/csrc/pmctl.hip.h PmctlLayout: what
// zh_pmctl_set_state and zh_pmctl_get_state run through span_voice.hip.h's voice_get_state / voice_set_state) as a stand-alone
// program for AddressSanitizer + UBSan, as lead_state_host.cpp and dual_state_host.cpp run the other layouts.  For n = 0, 1, 65 and
// 130 voices: structs -> rows in a heap block of EXACTLY the library's size (kWords * n words) -> structs again, every field
// compared on bits; and every word of every row is written exactly once, at [word][voice].
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zang_amd/csrc/pmctl.hip.h"

static int fail(const char *what, int a = 0, int b = 0) { printf("%s (%d, %d)\nFAIL\n", what, a, b); return 1; }

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

static int run(size_t n) {
    using LY = PmctlLayout;
    std::vector<zh_pmctl_state> in(n), out(n);
    for (size_t v = 0; v < n; v++) in[v] = make((uint32_t)v);
    const size_t words = (size_t)LY::kWords * n;
    uint32_t *w = new uint32_t[words];                                // exactly the library's size
    for (size_t i = 0; i < words; i++) w[i] = 0xDEADBEEFu;
    for (size_t v = 0; v < n; v++) LY::pack(in[v], w, n, v);
    for (size_t i = 0; i < words; i++)
        if (w[i] == 0xDEADBEEFu) { delete[] w; return fail("a word not written", (int)(i / (n ? n : 1)), (int)(i % (n ? n : 1))); }
    for (size_t v = 0; v < n; v++) {                                  // [word][voice]: row k holds voice v's word k at column v
        uint32_t want[kPmctlState];
        words_of(in[v], want);
        for (size_t k = 0; k < (size_t)kPmctlState; k++)
            if (w[k * n + v] != want[k]) { delete[] w; return fail("row layout", (int)v, (int)k); }
    }
    for (size_t v = 0; v < n; v++) LY::unpack(out[v], w, n, v);
    delete[] w;
    for (size_t v = 0; v < n; v++)
        if (memcmp(&in[v], &out[v], sizeof(zh_pmctl_state)) != 0) return fail("round trip", (int)v);
    return 0;
}

int main() {
    static_assert(kPmctlState == 12 && sizeof(zh_pmctl_state) == 48, "12 words per controlled voice");
    static_assert(PC_RATIO_T == 0 && PC_MULT_T == 3 && PC_CARRIER_T == 6 && PC_MODULATOR_T == 7 && PC_ENV_STATE == 8 && PC_ENV_START == 11,
                  "the rows follow the struct's fields");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130})
        if (run(n)) return 1;
    printf("PASS\n");
    return 0;
}
