// spectrum_host.cpp -- zang::Spectrum and zang::Spectrogram (include/zang_hip.hpp) from a compiled host, without Python: 66 voices of
// a fixed integer pattern (exact in f32, so tests/test_cpp_spectrum.py builds the same image), one DrawSpectrum plot and five
// DrawSpectrumFull columns at moving frame starts -- linear, linear, logarithmic x 3 into a width of 3, so the buffer is cleared
// once and drawindex wraps -- each result's bits folded into one FNV-1a checksum, printed as one word per line.
#include <cstdio>
#include <vector>

#include "zang_hip.hpp"

static uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}

int main() {
    try {
        constexpr uint32_t V = 66, F = 1024 + 8, W = 3, H = 5;
        zang::Context ctx(0);
        std::vector<float> host((size_t)V * F);                                   // [voice][frame]
        for (uint32_t v = 0; v < V; v++)
            for (uint32_t f = 0; f < F; f++) host[(size_t)v * F + f] = (float)((v * 131u + f * 71u + (f * f) % 29u) % 257u) / 128.0f - 1.0f;
        zang::Image samples(ctx, V, F);
        samples.upload(host);
        zang::Spectrum spectrum(ctx, V);
        const std::vector<float> rows = spectrum.plot(samples, 3).download();     // [voice][512]
        printf("plot %016llx\n", (unsigned long long)fnv1a(0xCBF29CE484222325ull, rows.data(), rows.size() * sizeof(float)));
        zang::Spectrogram gram(ctx, V, W, H);
        const bool logs[5] = {false, false, true, true, true};
        for (uint32_t b = 0; b < 5; b++) {
            gram.plot(samples, 2 * b, logs[b]);
            const std::vector<uint32_t> stored = gram.download(), scrolled = gram.scrolled();
            uint64_t h = fnv1a(0xCBF29CE484222325ull, stored.data(), stored.size() * 4);
            h = fnv1a(h, scrolled.data(), scrolled.size() * 4);
            printf("gram %u %u %016llx\n", b, gram.drawindex(), (unsigned long long)h);
        }
        std::vector<float> re_host((size_t)V * 64), im_host((size_t)V * 64);
        for (size_t i = 0; i < re_host.size(); i++) { re_host[i] = host[i]; im_host[i] = host[re_host.size() + i]; }
        zang::Image re(ctx, V, 64), im(ctx, V, 64);
        re.upload(re_host);
        im.upload(im_host);
        zang::fft(ctx, 32, re, im, 7);
        const std::vector<float> r = re.download(), i = im.download();
        uint64_t h = fnv1a(0xCBF29CE484222325ull, r.data(), r.size() * sizeof(float));
        printf("fft %016llx\n", (unsigned long long)fnv1a(h, i.data(), i.size() * sizeof(float)));
        printf("PASS\n");
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
