// The controlled voice's three-cursor walk (zang_amd/csrc/pmctl.hip.h pmctl_walk) on the host, for ASan + UBSan: the text both
// pmctl kernels run, over heap blocks of exactly the tables' sizes ([K][V] per array) and with the identity where the kernel takes
// the wave-wide minimum.  Reads one case from stdin and prints every event and segment of every voice.
//   in:  V K buf_start buf_end filler; then for each of the three streams (notes, ratio, multiplier) and each voice:
//        count, then min(count, K) x (start end nic).  Rows at and above a voice's count hold `filler` as start and end.
//   out: per voice "V <v>", then "B <stream> <row k> <nic>" / "E <stream>" / "S <f0> <f1> <mask>" in the walk's order; "PASS"
#include <stdint.h>
#include <stdio.h>
#include <inttypes.h>
#include <vector>
#include "../../zang_amd/csrc/pmctl.hip.h"

struct Stream {
    std::vector<uint32_t> count, start, end;
    std::vector<uint8_t> nic;
};

int main() {
    uint32_t V, K, S, E, filler;
    if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &V, &K, &S, &E, &filler) != 5 || K == 0 || E < S) return 2;
    Stream st[kPmctlStreams];
    for (Stream &s : st) {
        const size_t cells = (size_t)K * V;
        s.count.assign(V, 0); s.start.assign(cells, filler); s.end.assign(cells, filler); s.nic.assign(cells, 1);
        for (size_t v = 0; v < V; v++) {
            if (scanf("%" SCNu32, &s.count[v]) != 1) return 2;
            for (uint32_t k = 0; k < s.count[v] && k < K; k++) {      // a count above the table's rows: the rows it has
                uint32_t nic;
                const size_t i = (size_t)k * V + v;
                if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &s.start[i], &s.end[i], &nic) != 3) return 2;
                s.nic[i] = (uint8_t)nic;
            }
        }
    }
    auto view = [&](const Stream &s) { return PmctlTable{K, s.count.data(), s.start.data(), s.end.data(), s.nic.data()}; };
    const PmctlTable tn = view(st[PMCTL_NOTES]), tr = view(st[PMCTL_RATIO]), tm = view(st[PMCTL_MULT]);
    for (size_t v = 0; v < V; v++) {
        printf("V %zu\n", v);
        uint32_t at = S;
        bool ok = true;
        pmctl_walk(tn, tr, tm, V, v, true, S, E,
                   [](uint32_t ev) { return ev; },
                   [&](int s, size_t kv, bool nic) {
                       if (kv % V != v || kv / V >= K) ok = false;     // a row of this voice, inside the table
                       printf("B %d %zu %d\n", s, kv / V, nic ? 1 : 0);
                   },
                   [&](uint32_t f0, uint32_t f1, uint32_t mask) {
                       if (f0 != at || f1 <= f0 || f1 > E) ok = false;  // the segments tile [S, E) in order, none empty
                       at = f1;
                       printf("S %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", f0, f1, mask);
                   },
                   [&](int s) { printf("E %d\n", s); });
        if (!ok || at != E) { printf("FAIL: voice %zu's segments do not tile the buffer\n", v); return 1; }
    }
    // lanes that own no voice walk no row: one segment over the whole buffer, nothing active
    {
        uint32_t segs = 0, masks = 0, events = 0;
        pmctl_walk(tn, tr, tm, V, 0, false, S, E, [](uint32_t ev) { return ev; }, [&](int, size_t, bool) { events++; },
                   [&](uint32_t, uint32_t, uint32_t mask) { segs++; masks |= mask; }, [&](int) { events++; });
        if (events || masks || segs != (E > S ? 1u : 0u)) { printf("FAIL: an idle lane walked rows\n"); return 1; }
    }
    printf("PASS\n");
    return 0;
}
