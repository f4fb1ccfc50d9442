// module_spans_host.cpp -- the builtin modules' span paints from the C++ host API (include/zang_hip.hpp): a PulseOsc voice bank
// and a Sampler voice bank each painted over one per-voice sub-span table (mod::X::paint_spans, zh_<module>_paint_spans), frequency /
// output rate and loop per sub-span, against the oracle running one zo_<module>_paint per sub-span, voice by voice.  Prints PASS.
#include "zang_hip.hpp"
extern "C" {
#include "zang_oracle.h"
}

#include <cstdio>
#include <cstring>
#include <vector>

static constexpr uint32_t V = 96, F = 1024, K = 3;
static constexpr float SR = 48000.0f;

struct Table {   // [K][V] host arrays of the reference's Trigger output for one buffer
    std::vector<uint32_t> count = std::vector<uint32_t>(V), start = std::vector<uint32_t>(K * V), end = std::vector<uint32_t>(K * V);
    std::vector<uint8_t> nic = std::vector<uint8_t>(K * V);
};

static Table make_table(uint32_t seed) {
    Table t;
    uint32_t x = seed;
    auto rnd = [&](uint32_t n) { x = x * 1664525u + 1013904223u; return (x >> 8) % n; };
    for (uint32_t v = 0; v < V; v++) {
        const uint32_t k = rnd(K + 1);
        uint32_t prev = 0;
        for (uint32_t j = 0; j < k; j++) {
            const uint32_t s = prev + rnd((F - prev) / 2 + 1);
            const uint32_t e = j + 1 == k && rnd(3) == 0 ? F : s + rnd(F - s + 1);
            t.start[j * V + v] = s; t.end[j * V + v] = e; t.nic[j * V + v] = (uint8_t)rnd(2);
            prev = e;
        }
        t.count[v] = k;
    }
    return t;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b, const char *what) {
    if (a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * 4) == 0) { printf("%s: bit-exact\n", what); return true; }
    printf("%s: MISMATCH\n", what);
    return false;
}

int main() {
    zang::Context ctx(0);
    bool ok = true;
    const Table t = make_table(7);
    zang::DeviceArray<uint32_t> d_count(ctx, t.count), d_start(ctx, t.start), d_end(ctx, t.end);
    zang::DeviceArray<uint8_t> d_nic(ctx, t.nic);
    const zh_script_span_table table{K, 0, d_count.get(), d_start.get(), d_end.get(), d_nic.get()};

    // ---- PulseOsc: freq and color per sub-span
    {
        std::vector<float> freq(K * V), color(K * V);
        for (uint32_t i = 0; i < K * V; i++) { freq[i] = 40.0f + 13.0f * (float)(i % 157); color[i] = (float)(i % 11) / 10.0f; }
        zang::DeviceArray<float> d_freq(ctx, freq), d_color(ctx, color);
        zh_script_span_param sp[ZH_PULSEOSC_SPAN_FIELDS] = {};
        sp[ZH_PULSEOSC_SPAN_FREQ].f = d_freq.get();
        sp[ZH_PULSEOSC_SPAN_COLOR].f = d_color.get();
        mod::PulseOsc osc(ctx, V);
        zang::Image out(ctx, V, F);
        std::vector<float> ref((size_t)V * F, 0.25f);
        out.upload(ref);
        osc.paint_spans(zang::Span{0, F}, {out}, {}, mod::PulseOsc::Params{SR, 0, zang::constant(440.0f), zang::f32(0.5f)}, sp, table);
        for (uint32_t v = 0; v < V; v++) {
            zo_pulseosc st; zo_pulseosc_init(&st);
            for (uint32_t k = 0; k < t.count[v]; k++) {
                const uint32_t i = k * V + v;
                zo_cob c{ZO_COB_CONSTANT, freq[i], nullptr};
                zo_pulseosc_paint(&st, t.start[i], t.end[i], &ref[(size_t)v * F], SR, c, color[i]);
            }
        }
        ok = same_bits(out.download(), ref, "PulseOsc paint_spans") && ok;
    }

    // ---- Sampler: output rate (negative: backwards) and loop per sub-span, note_id_changed resets the play position
    {
        std::vector<uint8_t> pcm(600 * 2);
        for (size_t i = 0; i < pcm.size(); i++) pcm[i] = (uint8_t)(i * 37u + 11u);
        zang::DeviceArray<uint8_t> d_pcm(ctx, pcm);
        std::vector<float> rate(K * V);
        std::vector<uint32_t> loop(K * V);
        for (uint32_t i = 0; i < K * V; i++) { rate[i] = (i % 5 == 0 ? -1.0f : 1.0f) * (22050.0f + 701.0f * (float)(i % 53)); loop[i] = i % 3 != 0; }
        zang::DeviceArray<float> d_rate(ctx, rate);
        zang::DeviceArray<uint32_t> d_loop(ctx, loop);
        zh_script_span_param sp[ZH_SAMPLER_SPAN_FIELDS] = {};
        sp[ZH_SAMPLER_SPAN_SAMPLE_RATE].f = d_rate.get();
        sp[ZH_SAMPLER_SPAN_LOOP].u = d_loop.get();
        mod::Sampler smp(ctx, V);
        zang::Image out(ctx, V, F);
        std::vector<float> ref((size_t)V * F, 0.0f);
        mod::Sampler::Params p{};
        p.sample_rate = zang::f32(SR);
        p.sample = zh_sample{2, 44100, ZH_SAMPLE_S16_LSB, 0, d_pcm.get(), pcm.size()};
        p.channel = 1;
        smp.paint_spans(zang::Span{0, F}, {out}, {}, p, sp, table, ZH_PAINT_ZERO_FIRST);
        for (uint32_t v = 0; v < V; v++) {
            zo_sampler st; zo_sampler_init(&st);
            for (uint32_t k = 0; k < t.count[v]; k++) {
                const uint32_t i = k * V + v;
                zo_sampler_params op{rate[i], 2, 44100, ZO_SAMPLE_S16, pcm.data(), pcm.size(), 1, (int32_t)loop[i]};
                zo_sampler_paint(&st, t.start[i], t.end[i], &ref[(size_t)v * F], t.nic[i], &op);
            }
        }
        ok = same_bits(out.download(), ref, "Sampler paint_spans") && ok;
    }
    ctx.sync();
    printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
