// live_lane_host.cpp -- the live voice bank's per-lane steps (zang_amd/csrc/sched_lane.hip.h: zs_push_dispatch, zs_live_word,
// zs_live_keep around the unchanged zs_dispatch_one / zs_trigger_buffer) on the CPU, laid out as k_voice_bank_schedule_live lays
// them out ([slot][instrument] slots and lists, [word][voice] carried records); compiled with -fsanitize=address,undefined by
// tests/test_live_bank_host.py.  Three modes:
//   trigger            stdin: n_steps, then per step n_impulses and per impulse `frame note_id event_id param_bits`; every impulse a
//                      note-on pushed into one instrument of polyphony 1, 1,024-frame buffers.  stdout per step: `step k`, then
//                      `start end bits changed`.  (Event ids are the queue's own.)
//   dispatch P         stdin: n, then per impulse `frame note_id event_id note_on`, pushed in one buffer.  stdout: per slot its note ids.
//   bank IN OUT        IN (binary): u32 N, P, words, note_on_offset, max_rows, n_buffers, 0, 0; per buffer u32 out_len, m, then the batch
//                      sorted by instrument: u32 offsets[N + 1], frame[m]; u64 note_id[m]; u32 rec[m][words].
//                      OUT per buffer: u32 count[V], start[max_rows][V], end[max_rows][V], words[W][max_rows][V], u8 note_on[max_rows][V],
//                      changed[max_rows][V]; at the end u64 dropped sub-spans, u64 next_event_id[N], u32 flags[V], u64 slot_note[V],
//                      slot_event[V], u32 trig_has[V], u64 trig_note[V], u32 carried[W][V] (voice = instrument * P + slot).
#include "../../zang_amd/csrc/sched_lane.hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// N instruments of polyphony P with W-word records: the state a live bank keeps between buffers, and one buffer's step
struct Bank {
    uint32_t N, P, W, on_off;
    std::vector<uint32_t> flags, trig_has, carried, l_slot, l_frame, l_ev;
    std::vector<uint64_t> slot_note, slot_event, trig_note, next_id;
    uint64_t dropped = 0;
    Bank(uint32_t n, uint32_t p, uint32_t w, uint32_t on)
        : N(n), P(p), W(w), on_off(on), flags((size_t)n * p, 0), trig_has((size_t)n * p, 0), carried((size_t)n * p * w, 0), l_slot(kZsMaxImpulses * n),
          l_frame(kZsMaxImpulses * n), l_ev(kZsMaxImpulses * n), slot_note((size_t)n * p, 0), slot_event((size_t)n * p, 0), trig_note((size_t)n * p, 0),
          next_id(n, 1) {}
    // emit(voice, start, end, ev, changed, batch, carried)
    template <class Emit>
    void buffer(uint32_t out_len, const std::vector<uint32_t> &offsets, const std::vector<uint32_t> &frame, const std::vector<uint64_t> &ids,
                const std::vector<uint32_t> &rec, Emit &&emit) {
        const ZsSong batch{nullptr, ids.data(), rec.data(), W, on_off / 4, (on_off & 3u) * 8};
        const size_t V = (size_t)N * P;
        for (uint32_t i = 0; i < N; i++) {
            // slots [slot][instrument], lists [entry][instrument]: the strides of the kernel's LDS
            const ZsSlots sl{flags.data() + i, slot_note.data() + i, slot_event.data() + i, N, P};
            const ZsList list{l_slot.data() + i, l_frame.data() + i, l_ev.data() + i, N};
            const uint32_t listed = zs_push_dispatch(batch, frame.data(), offsets[i], offsets[i + 1], next_id[i], sl, list);
            for (uint32_t s = 0; s < P; s++) {
                const size_t v = (size_t)i * P + s;
                const ZsCarried c{carried.data() + v, V};
                ZsTrigger tr{trig_has[v], kZsCarried, trig_note[v]};
                zs_trigger_buffer(tr, batch, list, listed, s, out_len, [&](uint32_t a, uint32_t b, uint32_t ev, uint32_t ch) { emit(v, a, b, ev, ch, batch, c); });
                zs_live_keep(tr, batch, c);
                if (tr.has_note && tr.ev != kZsCarried) abort();
                trig_has[v] = tr.has_note; trig_note[v] = tr.note_id;
            }
        }
    }
};

static int mode_trigger() {
    unsigned n_steps = 0;
    if (scanf("%u", &n_steps) != 1) return 2;
    Bank bank(1, 1, 2, 4);
    for (unsigned s = 0; s < n_steps; s++) {
        unsigned n = 0;
        if (scanf("%u", &n) != 1) return 2;
        std::vector<uint32_t> offsets{0, n}, frame(n), rec(2 * (size_t)n);
        std::vector<uint64_t> ids(n);
        for (unsigned i = 0; i < n; i++) {
            unsigned long long id, eid;
            unsigned f, bits;
            if (scanf("%u %llu %llu %u", &f, &id, &eid, &bits) != 4) return 2;
            frame[i] = f; ids[i] = id; rec[2 * i] = bits; rec[2 * i + 1] = 1;
        }
        printf("step %u\n", s);
        bank.buffer(1024, offsets, frame, ids, rec, [&](size_t, uint32_t a, uint32_t b, uint32_t ev, uint32_t ch, const ZsSong &batch, const ZsCarried &c) {
            printf("%u %u %u %u\n", a, b, zs_live_word(batch, c, ev, 0), ch);
        });
    }
    return 0;
}

static int mode_dispatch(unsigned P) {
    unsigned n = 0;
    if (scanf("%u", &n) != 1 || P == 0) return 2;
    std::vector<uint32_t> offsets{0, n}, frame(n), rec(n);
    std::vector<uint64_t> ids(n);
    for (unsigned i = 0; i < n; i++) {
        unsigned long long id, eid;
        unsigned f, on;
        if (scanf("%u %llu %llu %u", &f, &id, &eid, &on) != 4) return 2;
        frame[i] = f; ids[i] = id; rec[i] = on ? 1 : 0;
    }
    Bank bank(1, P, 1, 0);
    const ZsSong batch{nullptr, ids.data(), rec.data(), 1, 0, 0};
    const ZsSlots sl{bank.flags.data(), bank.slot_note.data(), bank.slot_event.data(), 1, P};
    const ZsList list{bank.l_slot.data(), bank.l_frame.data(), bank.l_ev.data(), 1};
    const uint32_t listed = zs_push_dispatch(batch, frame.data(), 0, n, bank.next_id[0], sl, list);
    for (unsigned s = 0; s < P; s++) {
        printf("slot %u:", s);
        for (uint32_t i = zs_next_of(list, listed, s, 0); i < listed; i = zs_next_of(list, listed, s, i + 1)) printf(" %llu", (unsigned long long)ids[bank.l_ev[i]]);
        printf("\n");
    }
    return 0;
}

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int mode_bank(const char *in, const char *out) {
    FILE *fi = fopen(in, "rb");
    if (!fi) return 2;
    uint32_t h[8];
    if (fread(h, 4, 8, fi) != 8) return 2;
    const uint32_t N = h[0], P = h[1], W = h[2], on_off = h[3], rows = h[4], nb = h[5];
    if (W == 0 || W > kZsMaxWords || on_off >= W * 4 || P == 0) return 2;
    FILE *fo = fopen(out, "wb");
    if (!fo) return 2;
    Bank bank(N, P, W, on_off);
    const size_t V = (size_t)N * P, cells = (size_t)rows * V;
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t hb[2];
        if (fread(hb, 4, 2, fi) != 2) return 2;
        const uint32_t out_len = hb[0], m = hb[1];
        std::vector<uint32_t> offsets, frame, rec;
        std::vector<uint64_t> ids;
        if (!rd(fi, offsets, (size_t)N + 1) || !rd(fi, frame, m) || !rd(fi, ids, m) || !rd(fi, rec, (size_t)m * W)) return 2;
        if (offsets[0] != 0 || offsets[N] != m) return 2;
        std::vector<uint32_t> count(V, 0), start(cells, 0), end(cells, 0), words(cells * W, 0);
        std::vector<uint8_t> on(cells, 0), changed(cells, 0);
        bank.buffer(out_len, offsets, frame, ids, rec, [&](size_t v, uint32_t s, uint32_t e, uint32_t ev, uint32_t ch, const ZsSong &batch, const ZsCarried &c) {
            const uint32_t k = count[v];
            if (k >= rows) { bank.dropped++; return; }
            const size_t idx = (size_t)k * V + v;
            start[idx] = s; end[idx] = e;
            for (uint32_t w = 0; w < W; w++) words[w * cells + idx] = zs_live_word(batch, c, ev, w);
            on[idx] = zs_live_note_on(batch, c, ev) ? 1 : 0;
            changed[idx] = (uint8_t)ch;
            count[v] = k + 1;
        });
        if (!wr(fo, count) || !wr(fo, start) || !wr(fo, end) || !wr(fo, words) || !wr(fo, on) || !wr(fo, changed)) return 2;
    }
    fclose(fi);
    // the slots back in [instrument][slot] order, as the kernel stores them
    std::vector<uint32_t> flags(V);
    std::vector<uint64_t> note(V), event(V);
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t s = 0; s < P; s++) {
            flags[(size_t)i * P + s] = bank.flags[(size_t)s * N + i]; note[(size_t)i * P + s] = bank.slot_note[(size_t)s * N + i];
            event[(size_t)i * P + s] = bank.slot_event[(size_t)s * N + i];
        }
    if (fwrite(&bank.dropped, 8, 1, fo) != 1 || !wr(fo, bank.next_id) || !wr(fo, flags) || !wr(fo, note) || !wr(fo, event) || !wr(fo, bank.trig_has) ||
        !wr(fo, bank.trig_note) || !wr(fo, bank.carried))
        return 2;
    fclose(fo);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "trigger")) return mode_trigger();
    if (argc >= 3 && !strcmp(argv[1], "dispatch")) return mode_dispatch((unsigned)atoi(argv[2]));
    if (argc >= 4 && !strcmp(argv[1], "bank")) return mode_bank(argv[2], argv[3]);
    fprintf(stderr, "usage: trigger | dispatch P | bank IN OUT\n");
    return 2;
}
