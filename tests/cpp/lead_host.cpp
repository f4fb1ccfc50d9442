// lead_host.cpp -- zang::Porta and zang::Vibrato (include/zang_hip.hpp) from a compiled host, without Python: 66 voices with up to
// two sub-spans each whose freq and note_on differ, short patches, each voice painted twice through the span form (ADD, then
// ZERO_FIRST) and once plainly without the frequency image -- the images' and the state's bits folded into one FNV-1a checksum
// per voice.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zang_hip.hpp"

static uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}

constexpr uint32_t V = 66, K = 2, F = 64, S = 3, E = 60;

template <class Voice>
static int run(zang::Context &ctx, const char *name, const typename Voice::Params &p, const zh_script_span_param *sp, const zh_script_span_table &table) {
    Voice voice(ctx, V);
    zang::Image out(ctx, V, F), sync(ctx, V, F);
    zang::zero(ctx, zang::Span::init(0, F), out);
    zang::zero(ctx, zang::Span::init(0, F), sync);
    voice.paintSpans(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, p, sp, table);
    const std::vector<float> first = out.download();
    voice.paintSpans(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, p, sp, table, ZH_PAINT_ZERO_FIRST);
    voice.paint(zang::Span::init(S, E), {zh_buf(out), zh_buf{}}, zang::boolean(false), p);
    ctx.sync();
    const std::vector<float> img = out.download(), freq_img = sync.download();   // [voice][frame]
    std::vector<typename Voice::State> st(V);
    voice.getState(st.data());
    float peak = 0.0f, fpeak = 0.0f;
    for (float x : img) peak = x > peak ? x : (-x > peak ? -x : peak);
    for (float x : freq_img) fpeak = x > fpeak ? x : fpeak;
    if (!(peak > 0.05f) || !(fpeak > 100.0f)) { printf("%s: silence\nFAIL\n", name); return 1; }
    uint64_t h = fnv1a(0xCBF29CE484222325ull, first.data(), first.size() * sizeof(float));
    h = fnv1a(h, img.data(), img.size() * sizeof(float));
    h = fnv1a(h, freq_img.data(), freq_img.size() * sizeof(float));
    h = fnv1a(h, st.data(), st.size() * sizeof(typename Voice::State));
    printf("%s checksum %016llx\n", name, (unsigned long long)h);
    return 0;
}

int main() {
    try {
        zang::Context ctx(0);
        std::vector<uint32_t> count(V), start(K * V), end(K * V), on(K * V);
        std::vector<uint8_t> nic(K * V);
        std::vector<float> freq(K * V);
        for (uint32_t v = 0; v < V; v++) {
            count[v] = v % 3;
            start[v] = S + v % 5; end[v] = 30; start[V + v] = 30 + v % 7; end[V + v] = E;
            nic[v] = 1; nic[V + v] = (v / 2) % 2;
            for (uint32_t k = 0; k < K; k++) { freq[k * V + v] = 110.0f * (float)(1 + (v + k) % 5); on[k * V + v] = k == 0 || v % 4 != 0; }
        }
        zang::DeviceArray<uint32_t> d_count(ctx, count), d_start(ctx, start), d_end(ctx, end), d_on(ctx, on);
        zang::DeviceArray<uint8_t> d_nic(ctx, nic);
        zang::DeviceArray<float> d_freq(ctx, freq);
        const zh_script_span_table table{K, 0, d_count.get(), d_start.get(), d_end.get(), d_nic.get()};
        zh_script_span_param sp[ZH_PORTA_SPAN_FIELDS] = {};
        static_assert((int)ZH_PORTA_SPAN_FIELDS == (int)ZH_VIBRATO_SPAN_FIELDS, "one Params record");
        sp[ZH_PORTA_SPAN_FREQ].f = d_freq.get();
        sp[ZH_PORTA_SPAN_NOTE_ON].u = d_on.get();

        zang::Porta::Patch pp = zang::Porta::defaultPatch();
        if (pp.glide_curve != ZH_CURVE_CUBED || pp.glide != 0.5f || pp.release != 1.0f) { printf("default porta patch\nFAIL\n"); return 1; }
        pp.glide = 30.0f / 48000.0f; pp.attack = 15.0f / 48000.0f; pp.decay = 25.0f / 48000.0f; pp.release = 40.0f / 48000.0f;
        const zh_porta_params p{48000.0f, 0, zang::f32(220.0f), zang::boolean(true), pp};
        if (run<zang::Porta>(ctx, "porta", p, sp, table)) return 1;

        zang::Vibrato::Patch vp = zang::Vibrato::defaultPatch();
        if (vp.vib_hz != 4.0f || vp.depth != 0.02f || vp.color != 0.5f) { printf("default vibrato patch\nFAIL\n"); return 1; }
        vp.vib_hz = 400.0f; vp.depth = 0.3f; vp.color = 0.3f;
        const zh_vibrato_params q{48000.0f, 0, zang::f32(220.0f), zang::boolean(true), vp};
        if (run<zang::Vibrato>(ctx, "vibrato", q, sp, table)) return 1;
        printf("PASS\n");
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
