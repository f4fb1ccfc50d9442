// fft_lane_host.cpp -- the spectrum analyser's per-element arithmetic (zang_amd/csrc/fft_lane.hip.h) on the CPU: the same functions
// k_spectrum runs, compiled for the host with -fsanitize=address,undefined by tests/test_spectrum_host.py, driven the way the kernel
// drives them -- rows stored at their bit-reversed index, then stage after stage of zf_butterfly over the table of zf_twiddles -- on
// heap blocks of exactly the sizes used.  Two modes, both reading and writing little-endian binary files:
//   fft IN OUT     IN: u32 voices, n; f32 re[n][voices], im[n][voices].            OUT: f32 re[n][voices], im[n][voices]
//   plot IN OUT    IN: u32 voices, height; f32 samples[1024][voices].              OUT: f32 plot[512][voices], u32 column[height][voices]
// The column is the LINEAR one only: the logarithmic position goes through the library's pow (zmath.hip.h zpowf), which is device
// code and does not compile for the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zang_amd/csrc/fft_lane.hip.h"

static bool read_all(const char *path, std::vector<unsigned char> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

// fft(n, re, im) for one voice's column of two [n][voices] arrays
static void transform(uint32_t n, uint32_t voices, uint32_t v, const float *re_in, const float *im_in, float *re, float *im, const float *tw) {
    uint32_t log2n = 0;
    while ((1u << log2n) < n) log2n++;
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t at = zf_bit_reverse(r, log2n);
        re[at] = re_in[(size_t)r * voices + v];
        im[at] = im_in ? im_in[(size_t)r * voices + v] : 0.0f;
    }
    for (uint32_t l1 = 1; l1 < n; l1 <<= 1)
        for (uint32_t g = 0; g < n / 2; g++) {
            const uint32_t j = g & (l1 - 1), h = ((g - j) << 1) + j;
            const float *u = tw + 2 * (size_t)zf_twiddle_index(l1, j);
            zf_butterfly(re[h], im[h], re[h + l1], im[h + l1], u[0], u[1]);
        }
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: fft_lane_host fft|plot IN OUT\n"); return 2; }
    std::vector<unsigned char> in;
    if (!read_all(argv[2], in) || in.size() < 8) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    uint32_t head[2];
    memcpy(head, in.data(), 8);
    const uint32_t voices = head[0];
    const bool plot = strcmp(argv[1], "plot") == 0;
    const uint32_t n = plot ? kFftMaxN : head[1], height = plot ? head[1] : 0;
    if (n < 2 || n > kFftMaxN || (n & (n - 1)) || (plot && height < 2)) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t cells = (size_t)n * voices;
    if (in.size() != 8 + cells * 4 * (plot ? 1 : 2)) { fprintf(stderr, "bad size\n"); return 2; }
    std::vector<float> data((in.size() - 8) / 4);
    memcpy(data.data(), in.data() + 8, in.size() - 8);
    std::vector<float> tw(2 * (size_t)(n - 1));
    zf_twiddles(tw.data(), n);
    std::vector<float> re(n), im(n);
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    if (!plot) {
        std::vector<float> ore(cells), oim(cells);
        for (uint32_t v = 0; v < voices; v++) {
            transform(n, voices, v, data.data(), data.data() + cells, re.data(), im.data(), tw.data());
            for (uint32_t r = 0; r < n; r++) { ore[(size_t)r * voices + v] = re[r]; oim[(size_t)r * voices + v] = im[r]; }
        }
        fwrite(ore.data(), 4, cells, out);
        fwrite(oim.data(), 4, cells, out);
    } else {
        std::vector<float> rows((size_t)kSpectrumBins * voices);
        std::vector<uint32_t> pixels((size_t)height * voices);
        for (uint32_t v = 0; v < voices; v++) {
            transform(n, voices, v, data.data(), nullptr, re.data(), im.data(), tw.data());
            for (uint32_t k = 0; k < kSpectrumBins; k++) rows[(size_t)k * voices + v] = zf_plot_value(re[k]);
            for (uint32_t i = 0; i < height; i++) {
                const float value = zf_fft_value(zf_pixel_f(i, height), [&](uint32_t k) { return re[k]; });
                pixels[(size_t)(height - 1 - i) * voices + v] = zf_pixel(value);
            }
        }
        fwrite(rows.data(), 4, rows.size(), out);
        fwrite(pixels.data(), 4, pixels.size(), out);
    }
    fclose(out);
    printf("PASS\n");
    return 0;
}
