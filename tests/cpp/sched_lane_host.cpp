// sched_lane_host.cpp -- the voice bank's per-lane scheduling steps (zang_amd/csrc/sched_lane.hip.h) on the CPU: the
// same functions the kernel k_voice_bank_schedule runs, compiled for the host with -fsanitize=address,undefined by
// tests/test_voice_bank_host.py.  Three modes:
//   trigger            stdin: n_steps, then per step n_impulses and per impulse `frame note_id event_id param_bits`;
//                      1,024-frame buffers, one Trigger (slot 0).  stdout per step: `step k`, then `start end bits changed`.
//   dispatch P         stdin: n, then per impulse `frame note_id event_id note_on`.  stdout: per slot its note ids.
//   song IN OUT        IN (binary): u32 P, words, note_on_offset, n_events, sample_rate bits, max_rows, n_buffers, 0;
//                      u32 frames[n_buffers]; f32 t[n]; u64 note_id[n]; u32 rec[n][words].  One instrument, buffer by buffer.
//                      OUT per buffer: u32 count[P], start[max_rows][P], end[max_rows][P], words[W][max_rows][P],
//                      u8 note_on[max_rows][P], changed[max_rows][P]; at the end u64 dropped sub-spans.
#include "../../zang_amd/csrc/sched_lane.hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int mode_trigger() {
    unsigned n_steps = 0;
    if (scanf("%u", &n_steps) != 1) return 2;
    std::vector<uint64_t> ids;
    std::vector<uint32_t> rec;
    std::vector<float> t;
    ZsTrigger tr{0, 0, 0};
    for (unsigned s = 0; s < n_steps; s++) {
        unsigned n = 0;
        if (scanf("%u", &n) != 1 || n > kZsMaxImpulses) return 2;
        std::vector<uint32_t> slot(n, 0), frame(n), ev(n);
        for (unsigned i = 0; i < n; i++) {
            unsigned long long id, eid;
            unsigned f, bits;
            if (scanf("%u %llu %llu %u", &f, &id, &eid, &bits) != 4) return 2;
            frame[i] = f; ev[i] = (uint32_t)ids.size();
            ids.push_back(id); rec.push_back(bits); t.push_back(0.0f);
        }
        const ZsSong song{t.data(), ids.data(), rec.data(), 1, 0, 0};
        const ZsList list{slot.data(), frame.data(), ev.data(), 1};
        printf("step %u\n", s);
        zs_trigger_buffer(tr, song, list, n, 0, 1024, [&](uint32_t a, uint32_t b, uint32_t e, uint32_t changed) {
            printf("%u %u %u %u\n", a, b, rec[e], changed);
        });
    }
    return 0;
}

static int mode_dispatch(unsigned P) {
    unsigned n = 0;
    if (scanf("%u", &n) != 1 || n > kZsMaxImpulses || P == 0) return 2;
    std::vector<uint32_t> flags(P, 0), slot(n), frame(n), ev(n);
    std::vector<uint64_t> note(P, 0), event(P, 0), ids(n);
    const ZsSlots sl{flags.data(), note.data(), event.data(), 1, P};
    const ZsList list{slot.data(), frame.data(), ev.data(), 1};
    uint32_t listed = 0;
    for (unsigned i = 0; i < n; i++) {
        unsigned long long id, eid;
        unsigned f, on;
        if (scanf("%u %llu %llu %u", &f, &id, &eid, &on) != 4) return 2;
        ids[i] = id;
        listed = zs_dispatch_one(sl, list, listed, f, i, id, on != 0, eid);
    }
    for (unsigned s = 0; s < P; s++) {
        printf("slot %u:", s);
        for (uint32_t i = zs_next_of(list, listed, s, 0); i < listed; i = zs_next_of(list, listed, s, i + 1)) printf(" %llu", (unsigned long long)ids[ev[i]]);
        printf("\n");
    }
    return 0;
}

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int mode_song(const char *in, const char *out) {
    FILE *fi = fopen(in, "rb");
    if (!fi) return 2;
    uint32_t h[8];
    if (fread(h, 4, 8, fi) != 8) return 2;
    const uint32_t P = h[0], W = h[1], on_off = h[2], n = h[3], rows = h[5], nb = h[6];
    float sr;
    memcpy(&sr, &h[4], 4);
    std::vector<uint32_t> frames, rec;
    std::vector<float> t;
    std::vector<uint64_t> ids;
    if (!rd(fi, frames, nb) || !rd(fi, t, n) || !rd(fi, ids, n) || !rd(fi, rec, (size_t)n * W)) return 2;
    fclose(fi);
    FILE *fo = fopen(out, "wb");
    if (!fo) return 2;
    const ZsSong song{t.data(), ids.data(), rec.data(), W, on_off / 4, (on_off & 3u) * 8};
    std::vector<uint32_t> flags(P, 0), l_slot(kZsMaxImpulses), l_frame(kZsMaxImpulses), l_ev(kZsMaxImpulses);
    std::vector<uint64_t> note(P, 0), event(P, 0);
    std::vector<ZsTrigger> trig(P, ZsTrigger{0, 0, 0});
    const ZsSlots sl{flags.data(), note.data(), event.data(), 1, P};
    const ZsList list{l_slot.data(), l_frame.data(), l_ev.data(), 1};
    uint32_t next = 0;
    float clock = 0.0f;
    uint64_t dropped = 0;
    const size_t cells = (size_t)rows * P;
    for (uint32_t b = 0; b < nb; b++) {
        std::vector<uint32_t> count(P, 0), start(cells, 0), end(cells, 0), words(cells * W, 0);
        std::vector<uint8_t> on(cells, 0), changed(cells, 0);
        const uint32_t listed = zs_consume_dispatch(song, 0, n, next, clock, sr, frames[b], sl, list);
        for (uint32_t v = 0; v < P; v++) {
            uint32_t k = 0;
            zs_trigger_buffer(trig[v], song, list, listed, v, frames[b], [&](uint32_t s, uint32_t e, uint32_t ev, uint32_t ch) {
                if (k >= rows) { dropped++; return; }
                const size_t idx = (size_t)k * P + v;
                start[idx] = s; end[idx] = e;
                for (uint32_t w = 0; w < W; w++) words[w * cells + idx] = rec[(size_t)ev * W + w];
                on[idx] = zs_note_on(song, ev) ? 1 : 0;
                changed[idx] = (uint8_t)ch;
                k++;
            });
            count[v] = k;
        }
        if (!wr(fo, count) || !wr(fo, start) || !wr(fo, end) || !wr(fo, words) || !wr(fo, on) || !wr(fo, changed)) return 2;
    }
    if (fwrite(&dropped, 8, 1, fo) != 1) return 2;
    fclose(fo);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "trigger")) return mode_trigger();
    if (argc >= 3 && !strcmp(argv[1], "dispatch")) return mode_dispatch((unsigned)atoi(argv[2]));
    if (argc >= 4 && !strcmp(argv[1], "song")) return mode_song(argv[2], argv[3]);
    fprintf(stderr, "usage: trigger | dispatch P | song IN OUT\n");
    return 2;
}
