// fm_host.cpp -- zang::FMInstrument (include/zang_hip.hpp) from a compiled host, without Python: 130 voices in 26 instruments of 5
// painted over the spans [0, 200) and [200, 1024) -- the second with the notes released -- and the image's and the state's bits
// folded into one FNV-1a checksum, which tests/test_cpp_fm.py compares with the same paints made through ctypes.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zang_hip.hpp"

static uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}

int main() {
    try {
        constexpr uint32_t V = 130, G = 5, NI = V / G, F = 1024;
        const float sr = 48000.0f;
        zang::Context ctx(0);
        zang::FMInstrument fm(ctx, V, G);
        if (fm.instruments() != NI) { printf("instruments() = %u\nFAIL\n", fm.instruments()); return 1; }
        std::vector<zang::FMInstrument::Patch> patches(NI, zang::FMInstrument::defaultPatch());
        for (uint32_t j = 0; j < NI; j++) {
            patches[j].value[ZH_FM_MOD_FEEDBACK] = j % 8;
            patches[j].value[ZH_FM_ALGORITHM] = j % 2;
            patches[j].value[ZH_FM_CAR_WAVEFORM] = j % 4;
            patches[j].value[ZH_FM_MOD_ATTACK] = patches[j].value[ZH_FM_CAR_ATTACK] = 15;
            patches[j].value[ZH_FM_CAR_TREMOLO] = patches[j].value[ZH_FM_MOD_VIBRATO] = (j / 2) % 2;
        }
        fm.setPatches(patches);
        auto bad = patches;
        bad[NI - 1].value[ZH_FM_ALGORITHM] = 2;
        if (zh_fm_set_patches(fm.get(), bad.data(), NI) != ZH_ERR_INVALID) { printf("a bad patch value was accepted\nFAIL\n"); return 1; }
        std::vector<float> trem((size_t)NI * F), vib((size_t)NI * F), freq(V);     // [instrument][frame]
        for (uint32_t j = 0; j < NI; j++)
            for (uint32_t f = 0; f < F; f++) {
                trem[(size_t)j * F + f] = (float)((f * 7 + j * 3) % 101) / 101.0f - 0.5f;
                vib[(size_t)j * F + f] = (float)((f * 5 + j * 11) % 89) / 89.0f - 0.5f;
            }
        for (uint32_t v = 0; v < V; v++) freq[v] = 55.0f + 13.0f * (float)v;
        zang::Image out(ctx, V, F), ti(ctx, NI, F), vi(ctx, NI, F);
        ti.upload(trem); vi.upload(vib);
        zang::DeviceArray<float> freq_dev(ctx, freq);
        zang::zero(ctx, zang::Span::init(0, F), out);
        zang::FMInstrument::Params p{sr, 0, ti, vi, zang::f32(freq_dev), zang::boolean(true)};
        fm.paint(zang::Span::init(0, 200), {zh_buf(out)}, zang::boolean(true), p);
        p.note_on = zang::boolean(false);
        fm.paint(zang::Span::init(200, F), {zh_buf(out)}, zang::boolean(false), p);
        ctx.sync();
        const std::vector<float> img = out.download();                           // [voice][frame]
        const std::vector<zh_fm_state> st = fm.getState();
        float peak = 0.0f;
        for (float x : img) peak = x > peak ? x : (-x > peak ? -x : peak);
        if (!(peak > 0.05f)) { printf("silence\nFAIL\n"); return 1; }
        uint64_t h = fnv1a(0xCBF29CE484222325ull, img.data(), img.size() * sizeof(float));
        h = fnv1a(h, st.data(), st.size() * sizeof(zh_fm_state));
        printf("checksum %016llx\nPASS\n", (unsigned long long)h);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
