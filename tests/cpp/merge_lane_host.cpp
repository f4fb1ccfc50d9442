// The merge stage's lane walk (zang_amd/csrc/merge_lane.hip.h) on the host, for ASan + UBSan: the text k_span_merge runs, the row
// stores included, over heap blocks of exactly the library's sizes.  Reads one case from stdin and prints what the kernel would
// leave behind.
//   in:  n_players out_len max_spans rows(capacity) | n_fields_a on_a spans_a | n_fields_b on_b spans_b
//        per player: count_a, then min(count_a, spans_a) x (start end nic n_fields_a words); count_b, then the same for B
//        rows at and above a player's count: filler_start filler_end (given last on the first line), nic 1, words 0xdead0002
//   out: "dropped <total>" and per player "P <count>" + count x "R start end changed <n_a + n_b + 3 words>"
#include <stdint.h>
#include <stdio.h>
#include <inttypes.h>
#include <vector>
#include "../../zang_amd/csrc/merge_lane.hip.h"

struct Source {
    uint32_t nf, on, spans;
    std::vector<uint32_t> count, start, end, words;                   // [spans][n]; words [nf][spans][n]
    std::vector<uint8_t> nic;
};

static bool read_source(Source &s, size_t n, size_t p) {
    if (scanf("%" SCNu32, &s.count[p]) != 1) return false;
    for (uint32_t k = 0; k < s.count[p] && k < s.spans; k++) {                // a count above the table's rows: the rows it has
        const size_t i = (size_t)k * n + p;
        uint32_t nic;
        if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &s.start[i], &s.end[i], &nic) != 3) return false;
        s.nic[i] = (uint8_t)nic;
        for (uint32_t f = 0; f < s.nf; f++)
            if (scanf("%" SCNu32, &s.words[((size_t)f * s.spans + k) * n + p]) != 1) return false;
    }
    return true;
}

int main() {
    uint32_t n, out_len, max_spans, rows, filler_start, filler_end;
    Source a, b;
    if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32,
              &n, &out_len, &max_spans, &rows, &a.nf, &a.on, &a.spans, &b.nf, &b.on, &b.spans, &filler_start, &filler_end) != 12) return 2;
    if (a.nf == 0 || a.nf > kMergeMaxFields || b.nf == 0 || b.nf > kMergeMaxFields || a.on >= a.nf || b.on >= b.nf || max_spans == 0 ||
        max_spans > rows || a.spans == 0 || b.spans == 0) return 2;
    for (Source *s : {&a, &b}) {
        const size_t cells = (size_t)s->spans * n;
        s->count.assign(n, 0); s->start.assign(cells, filler_start); s->end.assign(cells, filler_end); s->nic.assign(cells, 1);
        s->words.assign(cells * s->nf, 0xdead0002u);
    }
    for (size_t p = 0; p < n; p++)
        if (!read_source(a, n, p) || !read_source(b, n, p)) return 2;
    auto view = [&](const Source &s) {
        MergeSrc m{s.spans, s.nf, s.count.data(), s.end.data(), s.nic.data(), nullptr, {nullptr, nullptr, nullptr, nullptr}};
        for (uint32_t f = 0; f < s.nf; f++) m.field[f] = s.words.data() + (size_t)f * s.spans * n;
        m.on = m.field[s.on];
        return m;
    };
    const MergeSrc A = view(a), B = view(b);
    // the stage's table, as span_merge.hip allocates it: `rows` is the capacity, max_spans what this schedule may fill
    const size_t plane = (size_t)rows * n;
    const uint32_t nf = a.nf + b.nf + kMergeOwnFields;
    std::vector<uint32_t> count(n), start(plane), end(plane), words(plane * nf, 0xfeedfeedu);
    std::vector<uint8_t> changed(plane);
    const MergeOut out{count.data(), start.data(), end.data(), changed.data(), words.data(), plane};
    uint64_t dropped = 0;
    for (size_t p = 0; p < n; p++) dropped += merge_lane(A, B, out, n, p, out_len, max_spans);   // k_span_merge's body
    printf("dropped %" PRIu64 "\n", dropped);
    for (size_t p = 0; p < n; p++) {
        printf("P %" PRIu32 "\n", count[p]);
        for (uint32_t k = 0; k < count[p]; k++) {
            const size_t i = (size_t)k * n + p;
            printf("R %" PRIu32 " %" PRIu32 " %u", start[i], end[i], (unsigned)changed[i]);
            for (uint32_t f = 0; f < nf; f++) printf(" %" PRIu32, words[(size_t)f * plane + i]);
            printf("\n");
        }
    }
    printf("PASS\n");
    return 0;
}
