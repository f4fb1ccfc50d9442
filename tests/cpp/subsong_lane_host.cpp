// The subsong stage's lane steps (zang_amd/csrc/subsong_lane.hip.h) on the host, for ASan + UBSan: the text k_subsong_schedule
// runs, over heap blocks of exactly the library's sizes.  Reads one case from stdin and prints what the kernel would leave behind.
//   in:  base_freq_bits out_len max_spans n_players n_buffers in_spans n_melodies n_events
//        n_melodies + 1 offsets
//        n_events x (t_bits note_id freq_bits note_on)
//        per buffer: sample_rate_bits, then per player: count, then count x (start end note_id_changed freq_bits note_on melody)
//   out: per buffer "B <buffer> dropped <total>" and per player "P <count> <7 state words>" + count x "R start end freq_bits
//        note_on changed"
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <inttypes.h>
#include <vector>
#include "../../zang_amd/csrc/subsong_lane.hip.h"

int main() {
    uint32_t base_bits, out_len, max_spans, n, n_buffers, in_spans, K, E;
    if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &base_bits, &out_len, &max_spans, &n,
              &n_buffers, &in_spans, &K, &E) != 8) return 2;
    const float base_freq = ss_float(base_bits);
    std::vector<uint32_t> offsets((size_t)K + 1), t(E), id_lo(E), id_hi(E), fr(E), on(E);   // the kit's rows, as subsong.hip lays them out
    for (auto &o : offsets) if (scanf("%" SCNu32, &o) != 1 || o > E) return 2;
    for (uint32_t e = 0; e < E; e++) {
        uint64_t id;
        if (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &t[e], &id, &fr[e], &on[e]) != 4) return 2;
        id_lo[e] = (uint32_t)id; id_hi[e] = (uint32_t)(id >> 32);
    }
    const SubsongKitP kit{K, offsets.data(), t.data(), id_lo.data(), id_hi.data(), fr.data(), on.data()};
    std::vector<uint32_t> state((size_t)kSubsongState * n);            // [word][player], as subsong.hip allocates it
    for (size_t p = 0; p < n; p++) { SubsongLane s; subsong_init(s, K); subsong_store(s, state.data(), n, p); }
    const size_t cells = (size_t)max_spans * n;
    std::vector<uint32_t> count(n), start(cells), end(cells), freq(cells), note_on(cells);
    std::vector<uint8_t> changed(cells);
    const size_t in_cells = (size_t)in_spans * n;
    for (uint32_t b = 0; b < n_buffers; b++) {
        uint32_t sr_bits;
        if (scanf("%" SCNu32, &sr_bits) != 1) return 2;
        const float sample_rate = ss_float(sr_bits);
        std::vector<uint32_t> in_count(n), in_start(in_cells), in_end(in_cells), in_on(in_cells), in_mel(in_cells);
        std::vector<float> in_freq(in_cells);
        std::vector<uint8_t> in_nic(in_cells);
        for (size_t p = 0; p < n; p++) {
            if (scanf("%" SCNu32, &in_count[p]) != 1 || in_count[p] > in_spans) return 2;
            for (uint32_t k = 0; k < in_count[p]; k++) {
                const size_t i = (size_t)k * n + p;
                uint32_t nic, fb;
                if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &in_start[i], &in_end[i], &nic, &fb, &in_on[i],
                          &in_mel[i]) != 6) return 2;
                in_nic[i] = (uint8_t)nic; in_freq[i] = ss_float(fb);
            }
        }
        uint64_t dropped = 0;
        for (size_t p = 0; p < n; p++) {                               // k_subsong_schedule's body
            SubsongLane s;
            subsong_load(s, state.data(), n, p);
            SubsongEmit emit{SubsongRowsP{start.data(), end.data(), freq.data(), note_on.data(), changed.data()}, n, p, max_spans, 0, 0};
            subsong_buffer(s, kit, base_freq, sample_rate, out_len, in_count[p], in_start.data() + p, in_end.data() + p, in_nic.data() + p,
                           in_freq.data() + p, in_on.data() + p, in_mel.data() + p, n, emit);
            count[p] = emit.k;
            dropped += emit.dropped;
            subsong_store(s, state.data(), n, p);
        }
        printf("B %" PRIu32 " dropped %" PRIu64 "\n", b, dropped);
        for (size_t p = 0; p < n; p++) {
            SubsongLane s;
            subsong_load(s, state.data(), n, p);
            printf("P %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu32 "\n", count[p], s.next, s.t_bits,
                   s.melody, s.has_note, s.note_id, s.freq_bits, s.note_on);
            for (uint32_t k = 0; k < count[p]; k++) {
                const size_t i = (size_t)k * n + p;
                printf("R %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %u\n", start[i], end[i], freq[i], note_on[i], (unsigned)changed[i]);
            }
        }
    }
    printf("PASS\n");
    return 0;
}
