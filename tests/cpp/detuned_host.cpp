// detuned_host.cpp -- zang::Detuned (include/zang_hip.hpp) from a compiled host, without Python: 66 voices with up to two
// sub-spans each whose freq, note_on and mode differ, a short patch, painted twice through the span form (ADD, then ZERO_FIRST)
// and once uniformly without the frequency image -- the images' and the state's bits folded into one FNV-1a checksum.
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
        constexpr uint32_t V = 66, K = 2, F = 64, S = 3, E = 60;
        zang::Context ctx(0);
        std::vector<uint32_t> count(V), start(K * V), end(K * V), on(K * V), mode(K * V);
        std::vector<uint8_t> nic(K * V);
        std::vector<float> freq(K * V);
        for (uint32_t v = 0; v < V; v++) {
            count[v] = v % 3;
            start[v] = S + v % 5; end[v] = 30; start[V + v] = 30 + v % 7; end[V + v] = E;
            nic[v] = 1; nic[V + v] = (v / 2) % 2;
            for (uint32_t k = 0; k < K; k++) { freq[k * V + v] = 110.0f * (float)(1 + (v + k) % 5); on[k * V + v] = k == 0 || v % 4 != 0; mode[k * V + v] = (v + k) % 4; }
        }
        zang::DeviceArray<uint32_t> d_count(ctx, count), d_start(ctx, start), d_end(ctx, end), d_on(ctx, on), d_mode(ctx, mode);
        zang::DeviceArray<uint8_t> d_nic(ctx, nic);
        zang::DeviceArray<float> d_freq(ctx, freq);
        const zh_script_span_table table{K, 0, d_count.get(), d_start.get(), d_end.get(), d_nic.get()};
        zh_script_span_param sp[ZH_DETUNED_SPAN_FIELDS] = {};
        sp[ZH_DETUNED_SPAN_FREQ].f = d_freq.get();
        sp[ZH_DETUNED_SPAN_NOTE_ON].u = d_on.get();
        sp[ZH_DETUNED_SPAN_MODE].u = d_mode.get();
        zang::Detuned voice(ctx, V, 1000);
        zang::Image out(ctx, V, F), sync(ctx, V, F);
        zang::zero(ctx, zang::Span::init(0, F), out);
        zang::zero(ctx, zang::Span::init(0, F), sync);
        zang::Detuned::Patch patch = zang::Detuned::defaultPatch();
        if (patch.cutoff_hz != 880.0f || patch.volume != 0.75f) { printf("default patch\nFAIL\n"); return 1; }
        patch.warble_hz = 400.0f; patch.attack = 15.0f / 48000.0f; patch.decay = 25.0f / 48000.0f; patch.release = 40.0f / 48000.0f; patch.res = 0.3f;
        const zh_detuned_params p{48000.0f, 0, zang::f32(220.0f), zang::boolean(true), zang::u32(0), patch};
        voice.paintSpans(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, p, sp, table);
        const std::vector<float> first = out.download();
        voice.paintSpans(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, p, sp, table, ZH_PAINT_ZERO_FIRST);
        voice.paint(zang::Span::init(S, E), {zh_buf(out), zh_buf{}}, zang::boolean(false), p);
        ctx.sync();
        const std::vector<float> img = out.download(), freq_img = sync.download();   // [voice][frame]
        std::vector<zh_detuned_state> st(V);
        voice.getState(st.data());
        float peak = 0.0f, fpeak = 0.0f;
        for (float x : img) peak = x > peak ? x : (-x > peak ? -x : peak);
        for (float x : freq_img) fpeak = x > fpeak ? x : fpeak;
        if (!(peak > 0.05f) || !(fpeak > 100.0f)) { printf("silence\nFAIL\n"); return 1; }
        uint64_t h = fnv1a(0xCBF29CE484222325ull, first.data(), first.size() * sizeof(float));
        h = fnv1a(h, img.data(), img.size() * sizeof(float));
        h = fnv1a(h, freq_img.data(), freq_img.size() * sizeof(float));
        h = fnv1a(h, st.data(), st.size() * sizeof(zh_detuned_state));
        printf("checksum %016llx\nPASS\n", (unsigned long long)h);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
