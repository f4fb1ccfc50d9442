// lead_state_host.cpp -- the two lead voices' state layouts (zang_amd/csrc/lead.hip.h ps_pack / ps_unpack, vs_pack / vs_unpack: what
// zh_porta_set_state, zh_vibrato_set_state and their get_state run) as a stand-alone program for AddressSanitizer + UBSan.  For
// n = 0, 1, 65 and 130 voices: structs -> rows in a heap block of EXACTLY the library's size (kWords * n words) -> structs again,
// every field compared on bits; and every word of every row is written exactly once, at [word][voice].
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zang_amd/csrc/lead.hip.h"

static int fail(const char *what, int a = 0, int b = 0) { printf("%s (%d, %d)\nFAIL\n", what, a, b); return 1; }

static zh_porta_state make_porta(uint32_t v) {
    zh_porta_state s;
    memset(&s, 0, sizeof(s));
    s.porta.t = 1.0f / (float)(v + 2); s.porta.last_value = 220.0f + (float)v; s.porta.start = ls_float(0x80000000u);
    s.env.state = v % 5; s.env.t = 1.0f / (float)(v + 1); s.env.last_value = ls_float(0x7FC00001u + v); s.env.start = ls_float(0x00000001u + v);
    s.osc.t = 0.25f * (float)v;
    s.prev_note_on = v & 1;
    return s;
}
static zh_vibrato_state make_vibrato(uint32_t v) {
    zh_vibrato_state s;
    memset(&s, 0, sizeof(s));
    s.vib.t = ls_float(0x7FC00001u + v);
    s.osc.cnt = 0xFFFFFFFFu - v;
    return s;
}

template <class LY, class Make, class Rows>
static int run(size_t n, Make make, Rows rows) {
    using State = typename LY::State;
    std::vector<State> in(n), out(n);
    for (size_t v = 0; v < n; v++) in[v] = make((uint32_t)v);
    const size_t words = (size_t)LY::kWords * n;
    uint32_t *w = new uint32_t[words];                                // exactly the library's size
    for (size_t i = 0; i < words; i++) w[i] = 0xDEADBEEFu;
    for (size_t v = 0; v < n; v++) LY::pack(in[v], w, n, v);
    for (size_t i = 0; i < words; i++)
        if (w[i] == 0xDEADBEEFu) { delete[] w; return fail("a word not written", (int)(i / (n ? n : 1)), (int)(i % (n ? n : 1))); }
    for (size_t v = 0; v < n; v++)                                    // [word][voice]: the rows hold voice v's value at column v
        if (!rows(in[v], w, n, v)) { delete[] w; return fail("row layout", (int)v); }
    for (size_t v = 0; v < n; v++) LY::unpack(out[v], w, n, v);
    delete[] w;
    for (size_t v = 0; v < n; v++)
        if (memcmp(&in[v], &out[v], sizeof(State)) != 0) return fail("round trip", (int)v);
    return 0;
}

int main() {
    static_assert(kPortaState == 9, "9 words per portamento voice");
    static_assert(kVibratoState == 2, "2 words per vibrato voice");
    static_assert(sizeof(zh_porta_state) == 36, "zh_porta_state");
    static_assert(sizeof(zh_vibrato_state) == 8, "zh_vibrato_state");
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)130}) {
        if (run<PortaLayout>(n, make_porta, [](const zh_porta_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)PS_ENV_STATE * n_ + v] == s.env.state && w[(size_t)PS_PREV_NOTE_ON * n_ + v] == s.prev_note_on &&
                       w[(size_t)PS_PORTA_START * n_ + v] == 0x80000000u && w[(size_t)PS_OSC_T * n_ + v] == ls_bits(s.osc.t) &&
                       w[(size_t)PS_PORTA_T * n_ + v] == ls_bits(s.porta.t);
            })) return 1;
        if (run<VibratoLayout>(n, make_vibrato, [](const zh_vibrato_state &s, const uint32_t *w, size_t n_, size_t v) {
                return w[(size_t)VS_OSC_CNT * n_ + v] == s.osc.cnt && w[(size_t)VS_VIB_T * n_ + v] == ls_bits(s.vib.t);
            })) return 1;
    }
    printf("PASS\n");
    return 0;
}
