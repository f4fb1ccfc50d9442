// state_harness.h -- what the stand-alone state-layout programs (tests/cpp/*_state_host.cpp) share: one fail(), one hostile() and
// one run<LY>(n, make, rows) over a Layout of zang_amd/csrc/state_block.hip.h (LY::State, LY::kWords, LY::pack, LY::unpack).
// Header-only and host-only; a program keeps its own make_*, row lambdas, static_asserts and voice counts.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

inline int fail(const char *what, int a = 0, int b = 0) { printf("%s (%d, %d)\nFAIL\n", what, a, b); return 1; }

// bit patterns a float field must carry untouched: NaN payloads (quiet and signalling), -0.0, denormals, all ones
inline float hostile(uint32_t v, uint32_t k) {
    uint32_t bits;
    switch ((v + k) % 6) {
    case 0: bits = 0x7FC00001u + v; break;
    case 1: bits = 0x80000000u; break;
    case 2: bits = 0x00000001u + v; break;
    case 3: bits = 0xFFFFFFFFu; break;
    case 4: bits = 0x7F800001u + 7 * v; break;
    default: bits = 0x807FFFFFu - v; break;
    }
    float f;
    memcpy(&f, &bits, sizeof(f));
    return f;
}

// n voices: make(v) structs -> rows in a heap block of EXACTLY the library's size (kWords * n words) -> structs again, compared on
// bits; every word of every row is written; rows(in, w, n, v) says whether the rows hold voice v's value at column v.  `prefill`:
// the structs read back start as 0xA5 bytes, so unpack must write every byte (off: they start zeroed, for a State with fields that
// are not part of the voice).
template <class LY, class Make, class Rows>
int run(size_t n, Make make, Rows rows, bool prefill = false) {
    using State = typename LY::State;
    std::vector<State> in(n), out(n);
    for (size_t v = 0; v < n; v++) in[v] = make((uint32_t)v);
    const size_t words = (size_t)LY::kWords * n;
    uint32_t *w = new uint32_t[words];                                // exactly the library's size
    std::vector<bool> marked(words, false);                           // (a value may itself be the marker: count only words that stay so under two markers)
    for (uint32_t marker : {0xDEADBEEFu, 0x21524110u}) {
        for (size_t i = 0; i < words; i++) w[i] = marker;
        for (size_t v = 0; v < n; v++) LY::pack(in[v], w, n, v);
        for (size_t i = 0; i < words; i++) {
            if (marker == 0xDEADBEEFu) marked[i] = w[i] == marker;
            else if (marked[i] && w[i] == marker) { delete[] w; return fail("a word not written", (int)(i / n), (int)(i % n)); }
        }
    }
    for (size_t v = 0; v < n; v++)                                    // [word][voice]: the rows hold voice v's value at column v
        if (!rows(in[v], w, n, v)) { delete[] w; return fail("row layout", (int)v); }
    for (size_t v = 0; v < n; v++) {
        if (prefill) memset(&out[v], 0xA5, sizeof(State));
        LY::unpack(out[v], w, n, v);
    }
    delete[] w;
    for (size_t v = 0; v < n; v++)
        if (memcmp(&in[v], &out[v], sizeof(State)) != 0) return fail("round trip", (int)v);
    return 0;
}
