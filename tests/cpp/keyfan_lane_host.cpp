// The key fan-out stage's lane steps (zang_amd/csrc/keyfan_lane.hip.h) and the stages' row writer (span_stage.hip.h) on the host,
// for ASan + UBSan: the text k_keyfan_schedule runs, over heap blocks of exactly the library's sizes.  Reads one case from stdin
// and prints what the kernel would leave behind.
//   in:  n_keys out_len max_spans n_players n_buffers in_spans
//        n_keys key frequencies as bits
//        per buffer, per player: count, then count x (start end held_lo held_hi)
//   out: per buffer "B <buffer> dropped <total>" and per voice "V <count> <6 state words>" + count x
//        "R start end freq_bits note_on changed note_on_byte"
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <inttypes.h>
#include <vector>
#include "../../zang_amd/csrc/keyfan_lane.hip.h"
#include "../../zang_amd/csrc/span_stage.hip.h"

int main() {
    uint32_t n_keys, out_len, max_spans, np, n_buffers, in_spans;
    if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &n_keys, &out_len, &max_spans, &np, &n_buffers, &in_spans) != 6)
        return 2;
    if (n_keys == 0 || n_keys > kKeyfanMaxKeys) return 2;
    std::vector<uint32_t> keys(n_keys);
    for (auto &k : keys) if (scanf("%" SCNu32, &k) != 1) return 2;
    const size_t nv = (size_t)np * n_keys;
    std::vector<uint32_t> state((size_t)kKeyfanState * nv);            // [word][voice], as keyfan.hip allocates it
    for (size_t v = 0; v < nv; v++) { KeyfanLane s; keyfan_init(s); keyfan_store(s, state.data(), nv, v); }
    const size_t cells = (size_t)max_spans * nv;                       // the stage's table at a capacity of max_spans rows
    std::vector<uint32_t> count(nv), start(cells), end(cells), words(2 * cells);
    std::vector<uint8_t> changed(cells), on8(cells);
    const StageRows table{count.data(), start.data(), end.data(), changed.data(), words.data(), cells};
    const uint32_t *freq = words.data(), *note_on = words.data() + cells;
    const size_t in_cells = (size_t)in_spans * np;
    for (uint32_t b = 0; b < n_buffers; b++) {
        std::vector<uint32_t> in_count(np), in_start(in_cells), in_end(in_cells), lo(in_cells), hi(in_cells);
        for (size_t p = 0; p < np; p++) {
            if (scanf("%" SCNu32, &in_count[p]) != 1 || in_count[p] > in_spans) return 2;
            for (uint32_t k = 0; k < in_count[p]; k++) {
                const size_t i = (size_t)k * np + p;
                if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &in_start[i], &in_end[i], &lo[i], &hi[i]) != 4) return 2;
            }
        }
        uint64_t dropped = 0;
        for (size_t v = 0; v < nv; v++) {                              // k_keyfan_schedule's body
            const uint32_t p = (uint32_t)(v / n_keys), key = (uint32_t)(v - (size_t)p * n_keys);
            KeyfanLane s;
            keyfan_load(s, state.data(), nv, v);
            StageWriterT<KeyfanRows> emit{KeyfanRows{table, table.start, table.end, on8.data()}, nv, v, max_spans, 0, 0};
            keyfan_buffer(s, keys[key], key, out_len, in_count[p], in_start.data() + p, in_end.data() + p, lo.data() + p, hi.data() + p, np, emit);
            count[v] = emit.k;
            dropped += emit.dropped;
            keyfan_store(s, state.data(), nv, v);
        }
        printf("B %" PRIu32 " dropped %" PRIu64 "\n", b, dropped);
        for (size_t v = 0; v < nv; v++) {
            KeyfanLane s;
            keyfan_load(s, state.data(), nv, v);
            printf("V %" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu32 "\n", count[v], s.next_id, s.down, s.has_note,
                   s.note_id, s.freq_bits, s.note_on);
            for (uint32_t k = 0; k < count[v]; k++) {
                const size_t i = (size_t)k * nv + v;
                printf("R %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %u %u\n", start[i], end[i], freq[i], note_on[i], (unsigned)changed[i], (unsigned)on8[i]);
            }
        }
    }
    printf("PASS\n");
    return 0;
}
