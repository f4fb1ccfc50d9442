// mix_groups_host.cpp -- zang::mixdownGroups / mixdownGroupsPcm (include/zang_hip.hpp) from a compiled host, without Python:
// 37 groups of 10 voices x 1,000 frames over the span [3, 997), against a plain C++ loop (bits) and against the calls they
// replace, zang::mixdownVoices(ZH_MIX_SEQUENTIAL) on each group's column view followed by zang::mixDown (bytes).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zang_hip.hpp"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uniform() {                     // xorshift64*, [0, 1)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return ((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

int main() {
    try {
        constexpr uint32_t G = 37, P = 10, V = G * P, F = 1000, A = 3, B = 997;
        const float vol = 0.25f;
        const zang::Span span = zang::Span::init(A, B);
        zang::Context ctx(0);
        std::vector<float> voices((size_t)V * F);             // [voice][frame]; sums of 10 reach both clamps at vol * 32767
        for (float &x : voices) x = (float)((uniform() * 2.0 - 1.0) * 1.6);
        voices[5 * F + 100] = NAN; voices[17 * F + 3] = INFINITY; voices[200 * F + 996] = -0.0f;
        zang::Image img(ctx, V, F);
        img.upload(voices);
        std::vector<float> start((size_t)G * F);
        for (float &x : start) x = (float)(uniform() - 0.5);
        // the plain loop
        std::vector<float> want(start);
        std::vector<uint8_t> want_pcm((size_t)G * F * 2, 0x5A);
        for (uint32_t g = 0; g < G; g++)
            for (uint32_t f = A; f < B; f++) {
                float s = start[(size_t)g * F + f];
                for (uint32_t k = 0; k < P; k++) s = s + voices[(size_t)(g * P + k) * F + f];
                want[(size_t)g * F + f] = s;
                const float value = s * (vol * 32767.0f);
                const int32_t c = value <= -32767.0f ? -32767 : value >= 32766.0f ? 32766 : value != value ? 0 : (int32_t)value;
                want_pcm[((size_t)g * F + f) * 2] = (uint8_t)(c & 0xFF);
                want_pcm[((size_t)g * F + f) * 2 + 1] = (uint8_t)((c >> 8) & 0xFF);
            }
        // the grouped calls: `+=` onto the start rows, and the PCM form with the start rows as acc
        zang::DeviceArray<float> rows(ctx, start), acc(ctx, start), seq(ctx, start);
        zang::DeviceArray<uint8_t> pcm(ctx, std::vector<uint8_t>((size_t)G * F * 2, 0x5A)), seq_pcm(ctx, std::vector<uint8_t>((size_t)G * F * 2, 0x5A));
        zang::mixdownGroups(ctx, span, rows.get(), F, img, P);
        zang::mixdownGroupsPcm(ctx, span, pcm.get(), (size_t)F * 2, img, P, acc.get(), F, ZH_AUDIO_SIGNED16_LSB, 1, 0, vol);
        // the calls they replace, group by group
        for (uint32_t g = 0; g < G; g++) {
            zh_buf view = img;
            view.ptr += (size_t)g * P;
            view.voices = P;
            zang::mixdownVoices(ctx, span, seq.get() + (size_t)g * F, view, ZH_MIX_SEQUENTIAL);
            zang::mixDown(ctx, seq_pcm.get() + ((size_t)g * F + A) * 2, seq.get() + (size_t)g * F + A, B - A, ZH_AUDIO_SIGNED16_LSB, 1, 0, vol);
        }
        ctx.sync();
        const auto got = rows.download(), got_seq = seq.download();
        const auto got_pcm = pcm.download(), got_seq_pcm = seq_pcm.download();
        size_t nans = 0, low = 0, high = 0;
        for (size_t i = 0; i < got.size(); i++) {
            const bool same = (got[i] != got[i] && want[i] != want[i]) || memcmp(&got[i], &want[i], 4) == 0;
            const bool same_seq = (got[i] != got[i] && got_seq[i] != got_seq[i]) || memcmp(&got[i], &got_seq[i], 4) == 0;
            if (!same || !same_seq) { printf("row %zu frame %zu: sums differ\nFAIL\n", i / F, i % F); return 1; }
            nans += got[i] != got[i];
        }
        for (size_t i = 0; i < got_pcm.size(); i++)
            if (got_pcm[i] != want_pcm[i] || got_pcm[i] != got_seq_pcm[i]) { printf("row %zu byte %zu: PCM differs\nFAIL\n", i / (F * 2), i % (F * 2)); return 1; }
        for (size_t i = 0; i + 1 < got_pcm.size(); i += 2) {
            const int16_t s = (int16_t)(got_pcm[i] | (got_pcm[i + 1] << 8));
            low += s == -32767; high += s == 32766;
        }
        if (!nans || !low || !high) { printf("no NaN or no clamped sample (%zu, %zu, %zu)\nFAIL\n", nans, low, high); return 1; }
        // refusals
        if (zh_mixdown_groups(ctx.get(), A, B, rows.get(), F, img, 7, 0) != ZH_ERR_INVALID ||
            zh_mixdown_groups(ctx.get(), A, B, rows.get(), F, img, P, ZH_PAINT_TOLERANT) != ZH_ERR_UNSUPPORTED ||
            zh_mixdown_groups_pcm(ctx.get(), A, B, pcm.get(), (size_t)F * 2, img, P, nullptr, 0, 2, 1, 0, vol) != ZH_ERR_INVALID) {
            printf("a refusal did not return its code\nFAIL\n");
            return 1;
        }
        printf("%u groups of %u voices x %u frames: sums bit-exact, PCM identical to the per-group calls (%zu NaN, %zu + %zu clamped)\nPASS\n", G, P, B - A,
               nans, low, high);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
