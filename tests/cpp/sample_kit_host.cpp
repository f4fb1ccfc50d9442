// sample_kit_host.cpp -- zang::SampleKit and mod::paintKitSpans (include/zang_hip.hpp) from a compiled host, without Python: a
// three-sample kit (u8 mono, s16 stereo, s24 mono with two stray bytes), 66 voices with up to two sub-spans each whose sample,
// channel, rate and loop flag differ, painted twice (ADD, then ZERO_FIRST) -- the image's and the state's bits folded into one
// FNV-1a checksum, which tests/test_cpp_sample_kit.py compares with the same paints made through ctypes.
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
        const uint32_t lens[3] = {37, 200, 125}, chans[3] = {1, 2, 1}, rates[3] = {44100, 22050, 48000};
        std::vector<std::vector<uint8_t>> bytes(3);
        std::vector<zh_sample> samples(3);
        for (uint32_t j = 0; j < 3; j++) {
            bytes[j].resize(lens[j]);
            for (uint32_t i = 0; i < lens[j]; i++) bytes[j][i] = (uint8_t)((i * 37 + j * 101 + 13) % 256);
            samples[j] = zh_sample{chans[j], rates[j], j, 0, bytes[j].data(), lens[j]};
        }
        zang::SampleKit kit(ctx, samples);
        if (kit.count() != 3 || kit.sample(2).data_len != 125 || !kit.sample(2).data) { printf("kit entries\nFAIL\n"); return 1; }
        std::vector<uint32_t> count(V), start(K * V), end(K * V), loop(K * V), smp(K * V), chn(K * V);
        std::vector<uint8_t> nic(K * V);
        std::vector<float> rate(K * V);
        const float rs[4] = {44100.0f, 22050.5f, -30000.0f, 48000.0f};
        for (uint32_t v = 0; v < V; v++) {
            count[v] = v % 3;
            start[v] = S + v % 5; end[v] = 30; start[V + v] = 30 + v % 7; end[V + v] = E;
            nic[v] = v % 2; nic[V + v] = (v / 2) % 2;
            for (uint32_t k = 0; k < K; k++) {
                smp[k * V + v] = (v + k) % 4; chn[k * V + v] = (v + k) % 2; rate[k * V + v] = rs[(v + 2 * k) % 4]; loop[k * V + v] = (v + k) % 2;
            }
        }
        zang::DeviceArray<uint32_t> d_count(ctx, count), d_start(ctx, start), d_end(ctx, end), d_loop(ctx, loop), d_smp(ctx, smp), d_chn(ctx, chn);
        zang::DeviceArray<uint8_t> d_nic(ctx, nic);
        zang::DeviceArray<float> d_rate(ctx, rate);
        const zh_script_span_table table{K, 0, d_count.get(), d_start.get(), d_end.get(), d_nic.get()};
        zh_script_span_param sp[ZH_SAMPLER_KIT_SPAN_FIELDS] = {};
        sp[ZH_SAMPLER_KIT_SPAN_SAMPLE_RATE].f = d_rate.get();
        sp[ZH_SAMPLER_KIT_SPAN_LOOP].u = d_loop.get();
        sp[ZH_SAMPLER_KIT_SPAN_SAMPLE].u = d_smp.get();
        sp[ZH_SAMPLER_KIT_SPAN_CHANNEL].u = d_chn.get();
        mod::Sampler sampler(ctx, V);
        zang::Image out(ctx, V, F);
        zang::zero(ctx, zang::Span::init(0, F), out);
        const zh_sampler_kit_params p{zang::f32(44100.0f), zang::boolean(false), zang::u32(0), zang::u32(0), kit.get()};
        mod::paintKitSpans(sampler, zang::Span::init(S, E), {zh_buf(out)}, p, sp, table);
        const std::vector<float> first = out.download();
        mod::paintKitSpans(sampler, zang::Span::init(S, E), {zh_buf(out)}, p, sp, table, ZH_PAINT_ZERO_FIRST);
        ctx.sync();
        const std::vector<float> img = out.download();                           // [voice][frame]
        std::vector<zh_sampler_state> st(V);
        zang::check(zh_sampler_get_state(sampler.get(), st.data()), "zh_sampler_get_state");
        float peak = 0.0f;
        for (float x : img) peak = x > peak ? x : (-x > peak ? -x : peak);
        if (!(peak > 0.05f)) { printf("silence\nFAIL\n"); return 1; }
        uint64_t h = fnv1a(0xCBF29CE484222325ull, first.data(), first.size() * sizeof(float));
        h = fnv1a(h, img.data(), img.size() * sizeof(float));
        h = fnv1a(h, st.data(), st.size() * sizeof(zh_sampler_state));
        printf("checksum %016llx\nPASS\n", (unsigned long long)h);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
