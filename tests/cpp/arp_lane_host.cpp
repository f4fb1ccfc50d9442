// The arpeggiator stage's lane steps (zang_amd/csrc/arp_lane.hip.h) on the host, for ASan + UBSan: the text k_arp_schedule runs,
// over heap blocks of exactly the library's sizes.  Reads one case from stdin and prints what the kernel would leave behind.
//   in:  sample_rate_bits n_keys out_len max_spans n_players n_buffers in_spans
//        n_keys key frequencies as bits
//        per buffer, per player: count, then count x (start end held_lo held_hi)
//   out: "invalid" if the sample rate is refused, else per buffer
//        "B <buffer> dropped <total>" and per player "P <count> <7 state words>" + count x "R start end freq_bits note_on changed"
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <inttypes.h>
#include <vector>
#include "../../zang_amd/csrc/arp_lane.hip.h"
#include "../../zang_amd/csrc/span_stage.hip.h"

int main() {
    uint32_t sr_bits, n_keys, out_len, max_spans, n, n_buffers, in_spans;
    if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &sr_bits, &n_keys, &out_len, &max_spans, &n,
              &n_buffers, &in_spans) != 7) return 2;
    float sample_rate;
    memcpy(&sample_rate, &sr_bits, 4);
    uint32_t nd = 0;
    if (!arp_note_duration(sample_rate, nd)) { printf("invalid\n"); return 0; }
    printf("nd %" PRIu32 "\n", nd);
    std::vector<uint32_t> keys(n_keys);
    for (auto &k : keys) if (scanf("%" SCNu32, &k) != 1) return 2;
    std::vector<uint32_t> state((size_t)kArpState * n);                // [word][player], as arp.hip allocates it
    for (size_t p = 0; p < n; p++) { ArpLane s; arp_init(s); arp_store(s, state.data(), n, p); }
    const size_t cells = (size_t)max_spans * n;                        // the stage's table at a capacity of max_spans rows
    std::vector<uint32_t> count(n), start(cells), end(cells), words(2 * cells);
    std::vector<uint8_t> changed(cells);
    const StageRows table{count.data(), start.data(), end.data(), changed.data(), words.data(), cells};
    const uint32_t *freq = words.data(), *note_on = words.data() + cells;
    const size_t in_cells = (size_t)in_spans * n;
    for (uint32_t b = 0; b < n_buffers; b++) {
        std::vector<uint32_t> in_count(n), in_start(in_cells), in_end(in_cells), lo(in_cells), hi(in_cells);
        for (size_t p = 0; p < n; p++) {
            if (scanf("%" SCNu32, &in_count[p]) != 1 || in_count[p] > in_spans) return 2;
            for (uint32_t k = 0; k < in_count[p]; k++) {
                const size_t i = (size_t)k * n + p;
                if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &in_start[i], &in_end[i], &lo[i], &hi[i]) != 4) return 2;
            }
        }
        uint64_t dropped = 0;
        for (size_t p = 0; p < n; p++) {                               // k_arp_schedule's body
            ArpLane s;
            arp_load(s, state.data(), n, p);
            StageWriter emit{table, n, p, max_spans, 0, 0};
            arp_buffer(s, keys.data(), n_keys, nd, out_len, in_count[p], in_start.data() + p, in_end.data() + p, lo.data() + p, hi.data() + p, n, emit);
            count[p] = emit.k;
            dropped += emit.dropped;
            arp_store(s, state.data(), n, p);
        }
        printf("B %" PRIu32 " dropped %" PRIu64 "\n", b, dropped);
        for (size_t p = 0; p < n; p++) {
            ArpLane s;
            arp_load(s, state.data(), n, p);
            printf("P %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRId32 " %" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu32 "\n", count[p], s.next_frame, s.next_id,
                   s.last_note, s.has_note, s.note_id, s.freq_bits, s.note_on);
            for (uint32_t k = 0; k < count[p]; k++) {
                const size_t i = (size_t)k * n + p;
                printf("R %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %u\n", start[i], end[i], freq[i], note_on[i], (unsigned)changed[i]);
            }
        }
    }
    printf("PASS\n");
    return 0;
}
