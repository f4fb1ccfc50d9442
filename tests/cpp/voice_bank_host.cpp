// voice_bank_host.cpp -- zang::VoiceBank (include/zang_hip.hpp) from a compiled host, without Python: 64 instruments of
// polyphony 4 scheduled on the device for 8 buffers, every table compared with per-instrument zh_poly_voice_schedule, and a
// PulseOsc + a NiceInstrument painted from the bank's views against the same paints from host-made, uploaded tables (bits).
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zang_hip.hpp"

struct NoteParams { float freq; uint8_t note_on; uint8_t pad[3]; };   // examples/example_song.zig MyNoteParams

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uniform() {                     // xorshift64*, (0, 1)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return ((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-12;
}

template <class T> static std::vector<T> down(zang::Context &c, const T *dev, size_t n) {
    std::vector<T> h(n);
    zang::check(zh_download(c.get(), h.data(), dev, n * sizeof(T)), "zh_download");
    return h;
}

int main() {
    try {
        constexpr uint32_t N = 64, P = 4, V = N * P, F = 1024, B = 8, ROWS = 34;
        const float SR = 48000.0f;
        zang::Context ctx(0);
        std::vector<uint64_t> offsets{0}, ids;
        std::vector<NoteParams> recs;
        std::vector<float> t;
        for (uint32_t i = 0; i < N; i++) {
            const double gap = i % 16 == 15 ? 0.0003 : 0.004;
            double now = 0.0;
            while (now < B * F / SR * 1.1) {
                now += gap * (0.2 + 1.6 * uniform());
                NoteParams p{};
                p.freq = (float)(50.0 + 1950.0 * uniform());
                p.note_on = uniform() < 0.6 ? 1 : 0;
                recs.push_back(p); t.push_back((float)now); ids.push_back(1 + (uint64_t)(uniform() * 6.0));
            }
            offsets.push_back(t.size());
        }
        zang::VoiceBank bank(ctx, P, offsetof(NoteParams, note_on), offsets, recs, t, ids);
        bank.reserve(ROWS);
        std::vector<zh_poly_voice *> host(N);
        for (uint32_t i = 0; i < N; i++)
            zang::check(zh_poly_voice_create(P, sizeof(NoteParams), offsetof(NoteParams, note_on), offsets[i + 1] - offsets[i], recs.data() + offsets[i],
                                             t.data() + offsets[i], ids.data() + offsets[i], &host[i]), "zh_poly_voice_create");
        mod::PulseOsc osc_h(ctx, V), osc_d(ctx, V);
        mod::NiceInstrument nice_h(ctx, V, zang::f32(0.25f)), nice_d(ctx, V, zang::f32(0.25f));
        zang::Image img_oh(ctx, V, F), img_od(ctx, V, F), img_nh(ctx, V, F), img_nd(ctx, V, F);
        const mod::PulseOsc::Params op{SR, 0, zang::constant(440.0f), zang::f32(0.5f)};
        const zang::Span span = zang::Span::init(0, F);
        size_t spans = 0;
        for (uint32_t b = 0; b < B; b++) {
            // the host's tables, assembled [row][voice]
            std::vector<uint32_t> count(V), start((size_t)ROWS * V), end((size_t)ROWS * V);
            std::vector<float> freq((size_t)ROWS * V);
            std::vector<uint8_t> on((size_t)ROWS * V), nic((size_t)ROWS * V);
            for (uint32_t i = 0; i < N; i++) {
                uint32_t c[P], s[ROWS * P], e[ROWS * P];
                NoteParams pr[ROWS * P];
                uint8_t ch[ROWS * P];
                const uint32_t frames = F;
                zang::check(zh_poly_voice_schedule(host[i], SR, &frames, 1, ROWS, c, s, e, pr, ch), "zh_poly_voice_schedule");
                for (uint32_t v = 0; v < P; v++) {
                    count[i * P + v] = c[v];
                    for (uint32_t k = 0; k < c[v]; k++) {
                        const size_t idx = (size_t)k * V + i * P + v;
                        start[idx] = s[k * P + v]; end[idx] = e[k * P + v]; freq[idx] = pr[k * P + v].freq; on[idx] = pr[k * P + v].note_on; nic[idx] = ch[k * P + v];
                    }
                }
            }
            bank.schedule(SR, {F}, ROWS);
            const zh_span_table tb = bank.spanTable(ROWS, 0);
            const auto d_count = down(ctx, tb.count, V);
            const auto d_start = down(ctx, tb.start, (size_t)ROWS * V), d_end = down(ctx, tb.end, (size_t)ROWS * V);
            const auto d_freq = down(ctx, tb.freq, (size_t)ROWS * V);
            const auto d_on = down(ctx, tb.note_on, (size_t)ROWS * V), d_nic = down(ctx, tb.note_id_changed, (size_t)ROWS * V);
            for (uint32_t v = 0; v < V; v++) {
                if (d_count[v] != count[v]) { printf("buffer %u voice %u: count %u != %u\nFAIL\n", b, v, d_count[v], count[v]); return 1; }
                for (uint32_t k = 0; k < count[v]; k++) {
                    const size_t idx = (size_t)k * V + v;
                    if (d_start[idx] != start[idx] || d_end[idx] != end[idx] || memcmp(&d_freq[idx], &freq[idx], 4) || d_on[idx] != on[idx] || d_nic[idx] != nic[idx]) {
                        printf("buffer %u voice %u sub-span %u differs\nFAIL\n", b, v, k);
                        return 1;
                    }
                    spans++;
                }
            }
            // the same paints from uploaded host tables and from the bank's views
            zang::DeviceArray<uint32_t> u_count(ctx, count), u_start(ctx, start), u_end(ctx, end);
            zang::DeviceArray<float> u_freq(ctx, freq);
            zang::DeviceArray<uint8_t> u_on(ctx, on), u_nic(ctx, nic);
            const zh_span_table htb{ROWS, 0, u_count.get(), u_start.get(), u_end.get(), u_freq.get(), u_on.get(), u_nic.get()};
            const zh_script_span_table hst{ROWS, 0, u_count.get(), u_start.get(), u_end.get(), u_nic.get()};
            const zh_script_span_param hsp[ZH_PULSEOSC_SPAN_FIELDS] = {{u_freq.get(), nullptr}, {nullptr, nullptr}};
            const zh_script_span_param dsp[ZH_PULSEOSC_SPAN_FIELDS] = {bank.spanParamF(0), {nullptr, nullptr}};
            osc_h.paint_spans(span, {img_oh}, {}, op, hsp, hst, ZH_PAINT_ZERO_FIRST);
            osc_d.paint_spans(span, {img_od}, {}, op, dsp, bank.scriptTable(ROWS), ZH_PAINT_ZERO_FIRST);
            mod::paintSpans(nice_h, span, {img_nh}, SR, htb, ZH_PAINT_ZERO_FIRST);
            mod::paintSpans(nice_d, span, {img_nd}, SR, tb, ZH_PAINT_ZERO_FIRST);
            ctx.sync();
            const auto a = img_oh.download(), c = img_od.download(), x = img_nh.download(), y = img_nd.download();
            if (memcmp(a.data(), c.data(), a.size() * 4) || memcmp(x.data(), y.data(), x.size() * 4)) { printf("buffer %u: images differ\nFAIL\n", b); return 1; }
        }
        const auto st = bank.getState();
        bank.setState(st);
        for (zh_poly_voice *h : host) zh_poly_voice_destroy(h);
        if (bank.overflows() != 0 || spans < (size_t)V * B / 2) { printf("overflows or too few sub-spans (%zu)\nFAIL\n", spans); return 1; }
        printf("%zu sub-spans of %u voices x %u buffers identical, 2 x %u images bit-exact\nPASS\n", spans, V, B, B);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
