// curve_player_host.cpp -- zang::SfxKit and zang::CurvePlayer (include/zang_hip.hpp) from a compiled host, without Python: the
// reference's pair of curves (zh_sfx_effect_curve_example) and a two-node linear pair in a kit, 66 voices with up to two sub-spans
// each whose effect and rel_freq differ, both outputs painted twice (ADD, then ZERO_FIRST) and once plainly -- both images' and
// the state's bits folded into one FNV-1a checksum.
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
        zh_curve_node example[9];
        std::vector<zh_sfx_effect> effects(2);
        zang::check(zh_sfx_effect_curve_example(&effects[0], example), "zh_sfx_effect_curve_example");
        const zh_curve_node ramp[2] = {{300.0f, 0.0f}, {900.0f, 0.001f}}, fall[2] = {{2000.0f, 0.0f}, {500.0f, 0.0005f}};
        effects[1] = zh_sfx_effect{{ramp, 2, ZH_CURVE_FN_LINEAR}, {fall, 2, ZH_CURVE_FN_SMOOTHSTEP}, {nullptr, 0, ZH_CURVE_FN_LINEAR}};
        zang::SfxKit kit(ctx, effects);
        if (kit.count() != 2 || kit.effect(0).carrier.count != 6 || kit.effect(1).volume.count != 0 || !kit.effect(1).carrier.nodes) {
            printf("kit entries\nFAIL\n");
            return 1;
        }
        std::vector<uint32_t> count(V), start(K * V), end(K * V), eff(K * V);
        std::vector<uint8_t> nic(K * V);
        std::vector<float> rel(K * V);
        for (uint32_t v = 0; v < V; v++) {
            count[v] = v % 3;
            start[v] = S + v % 5; end[v] = 30; start[V + v] = 30 + v % 7; end[V + v] = E;
            nic[v] = v % 2; nic[V + v] = (v / 2) % 2;
            for (uint32_t k = 0; k < K; k++) { eff[k * V + v] = (v + k) % 3; rel[k * V + v] = 0.75f + 0.25f * (float)((v + k) % 3); }
        }
        zang::DeviceArray<uint32_t> d_count(ctx, count), d_start(ctx, start), d_end(ctx, end), d_eff(ctx, eff);
        zang::DeviceArray<uint8_t> d_nic(ctx, nic);
        zang::DeviceArray<float> d_rel(ctx, rel);
        const zh_script_span_table table{K, 0, d_count.get(), d_start.get(), d_end.get(), d_nic.get()};
        zh_script_span_param sp[ZH_CURVE_PLAYER_SPAN_FIELDS] = {};
        sp[ZH_CURVE_PLAYER_SPAN_REL_FREQ].f = d_rel.get();
        sp[ZH_CURVE_PLAYER_SPAN_EFFECT].u = d_eff.get();
        zang::CurvePlayer voice(ctx, V);
        zang::Image out(ctx, V, F), sync(ctx, V, F);
        zang::zero(ctx, zang::Span::init(0, F), out);
        zang::zero(ctx, zang::Span::init(0, F), sync);
        const zh_curve_player_params p{48000.0f, 0, zang::f32(1.5f), zang::u32(0), kit.get()};
        voice.paintSpans(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, p, sp, table);
        const std::vector<float> first = out.download(), first_sync = sync.download();
        voice.paintSpans(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, p, sp, table, ZH_PAINT_ZERO_FIRST);
        voice.paint(zang::Span::init(S, E), {zh_buf(out), zh_buf(sync)}, zang::boolean(false), p);
        ctx.sync();
        const std::vector<float> img = out.download(), img_sync = sync.download();     // [voice][frame]
        std::vector<zh_curve_player_state> st(V);
        voice.getState(st.data());
        float peak = 0.0f, peak_sync = 0.0f;
        for (float x : img) peak = x > peak ? x : (-x > peak ? -x : peak);
        for (float x : img_sync) peak_sync = x > peak_sync ? x : peak_sync;
        if (!(peak > 0.05f) || !(peak_sync > 100.0f)) { printf("silence\nFAIL\n"); return 1; }
        uint64_t h = fnv1a(0xCBF29CE484222325ull, first.data(), first.size() * sizeof(float));
        h = fnv1a(h, first_sync.data(), first_sync.size() * sizeof(float));
        h = fnv1a(h, img.data(), img.size() * sizeof(float));
        h = fnv1a(h, img_sync.data(), img_sync.size() * sizeof(float));
        h = fnv1a(h, st.data(), st.size() * sizeof(zh_curve_player_state));
        printf("checksum %016llx\nPASS\n", (unsigned long long)h);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
