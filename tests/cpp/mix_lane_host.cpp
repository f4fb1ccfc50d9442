// mix_lane_host.cpp -- the grouped mixdown's per-(group, frame) arithmetic (zang_amd/csrc/mix_lane.hip.h, the text
// k_mix_groups / k_mix_groups_pcm run) compiled for the host, for AddressSanitizer + UBSan (tests/test_mix_groups_host.py).
//   mix_lane_host IN OUT
// IN:  11 uint32 words -- groups, P, frames, stride, span start, span end, zero_first, s16, num_channels, channel_index, vol (bits) --
//      then the image [frames][stride] f32, then the start rows [groups][frames] f32.
// OUT: the f32 form's rows [groups][frames] (start rows outside the span), then the PCM form's rows
//      [groups][frames * num_channels * bytes_per_sample], every byte the call does not own left at 0xAA.
// Every buffer is a heap block of exactly its size: a read or write past a row or a group is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zang_amd/csrc/mix_lane.hip.h"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: mix_lane_host IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    std::vector<uint32_t> h;
    if (!rd(in, h, 11)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t groups = h[0], P = h[1], frames = h[2], stride = h[3], start = h[4], end = h[5], zero_first = h[6], s16 = h[7], nch = h[8], ch = h[9];
    float vol;
    memcpy(&vol, &h[10], 4);
    if (stride < groups * P || end > frames || start > end || nch == 0 || ch >= nch) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> img, acc;
    // the last row ends with its last voice, as a view of a padded image may
    if (!rd(in, img, frames ? (size_t)(frames - 1) * stride + (size_t)groups * P : 0) || !rd(in, acc, (size_t)groups * frames)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(in);
    const uint32_t bps = s16 ? 2 : 1;
    std::vector<float> sums(acc);
    std::vector<uint8_t> pcm((size_t)groups * frames * nch * bps, 0xAA);
    const float mul = zm_pcm_mul(vol, s16 != 0);
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t f = start; f < end; f++) {
            const float s0 = zero_first ? 0.0f : acc[(size_t)g * frames + f];
            const float s = zm_add_ordered(s0, img.data() + (size_t)f * stride + (size_t)g * P, P, 1);
            sums[(size_t)g * frames + f] = s;
            const int32_t c = zm_pcm(s, mul, s16 != 0);
            uint8_t *p = pcm.data() + ((size_t)g * frames * nch + (size_t)f * nch + ch) * bps;
            if (s16) { p[0] = (uint8_t)(c & 0xFF); p[1] = (uint8_t)((c >> 8) & 0xFF); }
            else p[0] = (uint8_t)(int8_t)c;
        }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    const bool ok = (sums.empty() || fwrite(sums.data(), 4, sums.size(), out) == sums.size()) &&
                    (pcm.empty() || fwrite(pcm.data(), 1, pcm.size(), out) == pcm.size());
    fclose(out);
    return ok ? 0 : 2;
}
