// sample_kit_lane_host.cpp -- the sample kit's lane (zang_amd/csrc/sample_kit.hip.h SamplerKitLane, the text k_sampler_kit_spans
// runs per voice) and the kit's layout (zk_describe / zk_pack, the functions zh_sample_kit_create calls) compiled for the host,
// for AddressSanitizer + UBSan (tests/test_sample_kit_host.py).
//   sample_kit_lane_host IN OUT
// IN:  8 uint32 words -- samples, voices V, max_spans K, image rows, span start, span end, zero_first, 0 -- then per sample four
//      uint32 (num_channels, sample_rate, format, data_len) and, after all of them, the samples' bytes back to back; t [V] f32;
//      count [V]; start, end, note_id_changed [K][V] uint32; sample_rate [K][V] f32; loop, sample, channel [K][V] uint32; the
//      image [V][rows] f32.
// OUT: the image [V][rows] f32, then t [V] f32.
// The blob is a heap block of exactly the size the library allocates: a read past the last sample is a sanitizer report.
// The walk over a voice's sub-spans is the span paints' contract (zang_amd/csrc/span_walk.hip.h), one voice after the other.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zang_amd/csrc/sample_kit.hip.h"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: sample_kit_lane_host IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    std::vector<uint32_t> h, sh;
    if (!rd(in, h, 8)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t ns = h[0], V = h[1], K = h[2], rows = h[3], start = h[4], end = h[5], zf = h[6];
    if (start > end || end > rows || !rd(in, sh, (size_t)ns * 4)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<std::vector<uint8_t>> bytes(ns);
    std::vector<zh_sample> samples(ns);
    for (uint32_t i = 0; i < ns; i++) {
        if (!rd(in, bytes[i], sh[i * 4 + 3])) { fprintf(stderr, "short sample\n"); return 2; }
        samples[i] = zh_sample{sh[i * 4], sh[i * 4 + 1], sh[i * 4 + 2], 0, bytes[i].empty() ? nullptr : bytes[i].data(), bytes[i].size()};
    }
    std::vector<float> t, rate, img;
    std::vector<uint32_t> count, s0, s1, nic, loop, smp, chn;
    const size_t KV = (size_t)K * V;
    if (!rd(in, t, V) || !rd(in, count, V) || !rd(in, s0, KV) || !rd(in, s1, KV) || !rd(in, nic, KV) || !rd(in, rate, KV) || !rd(in, loop, KV) ||
        !rd(in, smp, KV) || !rd(in, chn, KV) || !rd(in, img, (size_t)V * rows)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(in);

    std::vector<ZkSampleDesc> desc(ns);
    size_t blob_bytes = 0;
    if (zk_describe(samples.data(), ns, desc.data(), &blob_bytes) != ZH_OK) { fprintf(stderr, "zk_describe refused the kit\n"); return 2; }
    uint8_t *blob = static_cast<uint8_t *>(malloc(blob_bytes));      // exactly the blob: nothing after it may be read
    if (!blob) return 2;
    zk_pack(samples.data(), ns, desc.data(), blob, blob_bytes);

    for (uint32_t v = 0; v < V; v++) {
        float *row = img.data() + (size_t)v * rows;
        SamplerKitLane o;
        o.idle();
        o.t = t[v];
        auto zero = [&](uint32_t a, uint32_t b) { if (zf) for (uint32_t f = a; f < b; f++) row[f] = 0.0f; };
        uint32_t i = start;
        const uint32_t cnt = count[v] < K ? count[v] : K;
        for (uint32_t k = 0; k < cnt; k++) {
            const size_t kv = (size_t)k * V + v;
            if (s0[kv] < i || s0[kv] > end) break;                    // never reached in order: the voice's list ends
            zero(i, s0[kv]);
            o.begin(desc.data(), ns, smp[kv], chn[kv], rate[kv], loop[kv] != 0, nic[kv] != 0);
            const bool ends = s1[kv] >= s0[kv] && s1[kv] <= end;
            const uint32_t seg_end = ends ? s1[kv] : end;
            for (uint32_t f = s0[kv]; f < seg_end; f++) {
                float val = 0.0f;
                const bool painted = o.frame(blob, val);
                const float base = zf ? 0.0f : row[f];
                if (painted) row[f] = base + val; else if (zf) row[f] = 0.0f;
            }
            i = seg_end;
            if (!ends) break;
            o.end();
        }
        zero(i, end);
        t[v] = o.t;
    }
    free(blob);
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    const bool ok = (img.empty() || fwrite(img.data(), 4, img.size(), out) == img.size()) && (t.empty() || fwrite(t.data(), 4, t.size(), out) == t.size());
    fclose(out);
    return ok ? 0 : 2;
}
