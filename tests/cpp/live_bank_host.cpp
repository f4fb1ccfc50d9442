// live_bank_host.cpp -- zang::LiveVoiceBank (include/zang_hip.hpp) from a compiled host, without Python: 65 instruments of
// polyphony 3 take pushed impulses for 8 buffers (one instrument in 16 pushes 40 per buffer, some pushes out of order, some at
// or above the buffer's end); every table is compared with the host classes composed per instrument (zh_impulse_queue_* ->
// zh_polyphony_dispatcher_dispatch -> zh_trigger_*), a NiceInstrument painted from the bank's view against the same paint from
// a host-made, uploaded table (bits), and the state saved in the middle restores the stream in a second bank.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zang_hip.hpp"

struct NoteParams { float freq; uint8_t note_on; uint8_t pad[3]; uint32_t serial; };

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uniform() {                     // xorshift64*, (0, 1)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return ((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-12;
}

template <class T> static std::vector<T> down(zang::Context &c, const T *dev, size_t n) {
    std::vector<T> h(n);
    zang::check(zh_download(c.get(), h.data(), dev, n * sizeof(T)), "zh_download");
    return h;
}

struct Tables { std::vector<uint32_t> count, start, end; std::vector<float> freq; std::vector<uint8_t> on, nic; };

template <class Bank> static Tables download(zang::Context &ctx, Bank &bank, uint32_t rows, uint32_t V) {
    const zh_span_table tb = bank.spanTable(rows, 0);
    return Tables{down(ctx, tb.count, V), down(ctx, tb.start, (size_t)rows * V), down(ctx, tb.end, (size_t)rows * V), down(ctx, tb.freq, (size_t)rows * V),
                  down(ctx, tb.note_on, (size_t)rows * V), down(ctx, tb.note_id_changed, (size_t)rows * V)};
}

static bool same(const Tables &a, const Tables &b, uint32_t V, const char *what, uint32_t buffer, size_t *spans) {
    for (uint32_t v = 0; v < V; v++) {
        if (a.count[v] != b.count[v]) { printf("%s, buffer %u voice %u: count %u != %u\nFAIL\n", what, buffer, v, a.count[v], b.count[v]); return false; }
        for (uint32_t k = 0; k < b.count[v]; k++) {
            const size_t idx = (size_t)k * V + v;
            if (a.start[idx] != b.start[idx] || a.end[idx] != b.end[idx] || memcmp(&a.freq[idx], &b.freq[idx], 4) || a.on[idx] != b.on[idx] || a.nic[idx] != b.nic[idx]) {
                printf("%s, buffer %u voice %u sub-span %u differs\nFAIL\n", what, buffer, v, k);
                return false;
            }
            if (spans) *spans += 1;
        }
    }
    return true;
}

int main() {
    try {
        constexpr uint32_t N = 65, P = 3, V = N * P, F = 1024, B = 8, ROWS = 34, HALF = 4;
        const float SR = 48000.0f;
        zang::Context ctx(0);
        zang::LiveVoiceBank<NoteParams> bank(ctx, N, P, offsetof(NoteParams, note_on), N * 40), second(ctx, N, P, offsetof(NoteParams, note_on), N * 40);
        bank.reserve(ROWS); second.reserve(ROWS);
        std::vector<zh_impulse_queue *> queue(N);
        std::vector<zh_polyphony_dispatcher *> disp(N);
        std::vector<zh_trigger *> trig(V);
        for (uint32_t i = 0; i < N; i++) {
            zang::check(zh_impulse_queue_create(sizeof(NoteParams), &queue[i]), "zh_impulse_queue_create");
            zang::check(zh_polyphony_dispatcher_create(P, sizeof(NoteParams), offsetof(NoteParams, note_on), &disp[i]), "zh_polyphony_dispatcher_create");
        }
        for (uint32_t v = 0; v < V; v++) zang::check(zh_trigger_create(sizeof(NoteParams), &trig[v]), "zh_trigger_create");
        mod::NiceInstrument nice_h(ctx, V, zang::f32(0.25f)), nice_d(ctx, V, zang::f32(0.25f));
        zang::Image img_h(ctx, V, F), img_d(ctx, V, F);
        const zang::Span span = zang::Span::init(0, F);
        const zh_span_table view = bank.spanTable(ROWS, 0);
        zang::LiveVoiceBank<NoteParams>::State saved;
        struct Push { uint32_t instrument, frame; uint64_t note_id; NoteParams rec; };
        std::vector<std::vector<Push>> later;                    // the pushes of the buffers after the state was saved
        std::vector<Tables> later_tables;
        size_t spans = 0;
        uint32_t serial = 1;
        for (uint32_t b = 0; b < B; b++) {
            // this buffer's pushes: instruments take turns, each instrument's frames mostly ascending
            std::vector<Push> pushes;
            std::vector<uint32_t> left(N), at(N, 0);
            uint32_t total = 0;
            for (uint32_t i = 0; i < N; i++) { left[i] = i % 16 == 15 ? 40 : (uint32_t)(uniform() * 7.0); total += left[i]; }
            while (total) {
                const uint32_t i = (uint32_t)(uniform() * N) % N;
                if (!left[i]) continue;
                const double u = uniform();
                uint32_t f = at[i] + (uint32_t)(uniform() * (i % 16 == 15 ? 50.0 : 400.0));
                if (u < 0.05 && at[i] > 0) f = at[i] - 1 - (uint32_t)(uniform() * (at[i] - 1));    // below its predecessor's
                else if (u < 0.20) f = at[i];
                else if (u < 0.25) f = F - 1;
                else if (u < 0.28) f = F + (uint32_t)(uniform() * 3.0);                          // at or above the buffer's end
                NoteParams p{};
                p.freq = (float)(50.0 + 1950.0 * uniform()); p.note_on = uniform() < 0.6 ? 1 : 0; p.serial = serial++;
                pushes.push_back(Push{i, f, 1 + (uint64_t)(uniform() * 6.0), p});
                if (f >= at[i]) at[i] = f;
                left[i]--; total--;
            }
            // the host classes, per instrument
            Tables ref{std::vector<uint32_t>(V), std::vector<uint32_t>((size_t)ROWS * V), std::vector<uint32_t>((size_t)ROWS * V), std::vector<float>((size_t)ROWS * V),
                       std::vector<uint8_t>((size_t)ROWS * V), std::vector<uint8_t>((size_t)ROWS * V)};
            for (const Push &p : pushes) zang::check(zh_impulse_queue_push(queue[p.instrument], p.frame, p.note_id, &p.rec), "zh_impulse_queue_push");
            for (uint32_t i = 0; i < N; i++) {
                zh_iap iap, poly[P];
                zang::check(zh_impulse_queue_consume(queue[i], &iap), "zh_impulse_queue_consume");
                zang::check(zh_polyphony_dispatcher_dispatch(disp[i], iap, poly), "zh_polyphony_dispatcher_dispatch");
                for (uint32_t s = 0; s < P; s++) {
                    const uint32_t v = i * P + s;
                    zang::check(zh_trigger_counter(trig[v], 0, F, poly[s]), "zh_trigger_counter");
                    zh_paint_span ps;
                    int rc;
                    uint32_t k = 0;
                    while ((rc = zh_trigger_next(trig[v], &ps)) == 1) {
                        if (k >= ROWS) { printf("more sub-spans than rows\nFAIL\n"); return 1; }
                        NoteParams np;
                        memcpy(&np, ps.params, sizeof np);
                        const size_t idx = (size_t)k * V + v;
                        ref.start[idx] = (uint32_t)ps.start; ref.end[idx] = (uint32_t)ps.end; ref.freq[idx] = np.freq; ref.on[idx] = np.note_on ? 1 : 0;
                        ref.nic[idx] = (uint8_t)ps.note_id_changed;
                        k++;
                    }
                    zang::check(rc, "zh_trigger_next");
                    ref.count[v] = k;
                }
            }
            // the bank
            if (b == HALF) saved = bank.getState();
            for (const Push &p : pushes) bank.push(p.instrument, p.frame, p.note_id, p.rec);
            bank.schedule(F, ROWS);
            const Tables got = download(ctx, bank, ROWS, V);
            if (!same(got, ref, V, "bank", b, &spans)) return 1;
            if (b >= HALF) { later.push_back(pushes); later_tables.push_back(got); }
            // the same paint from an uploaded host table and from the bank's view
            zang::DeviceArray<uint32_t> u_count(ctx, ref.count), u_start(ctx, ref.start), u_end(ctx, ref.end);
            zang::DeviceArray<float> u_freq(ctx, ref.freq);
            zang::DeviceArray<uint8_t> u_on(ctx, ref.on), u_nic(ctx, ref.nic);
            const zh_span_table htb{ROWS, 0, u_count.get(), u_start.get(), u_end.get(), u_freq.get(), u_on.get(), u_nic.get()};
            mod::paintSpans(nice_h, span, {img_h}, SR, htb, ZH_PAINT_ZERO_FIRST);
            mod::paintSpans(nice_d, span, {img_d}, SR, view, ZH_PAINT_ZERO_FIRST);
            ctx.sync();
            const auto x = img_h.download(), y = img_d.download();
            if (memcmp(x.data(), y.data(), x.size() * 4)) { printf("buffer %u: images differ\nFAIL\n", b); return 1; }
        }
        // a second bank takes the stream over from the saved state
        second.setState(saved);
        for (size_t j = 0; j < later.size(); j++) {
            for (const Push &p : later[j]) second.push(p.instrument, p.frame, p.note_id, p.rec);
            second.schedule(F, ROWS);
            if (!same(download(ctx, second, ROWS, V), later_tables[j], V, "restored bank", HALF + (uint32_t)j, nullptr)) return 1;
        }
        for (zh_impulse_queue *q : queue) zh_impulse_queue_destroy(q);
        for (zh_polyphony_dispatcher *d : disp) zh_polyphony_dispatcher_destroy(d);
        for (zh_trigger *t : trig) zh_trigger_destroy(t);
        if (bank.overflows() != 0 || second.overflows() != 0 || spans < (size_t)V * B / 2) { printf("overflows or too few sub-spans (%zu)\nFAIL\n", spans); return 1; }
        printf("%zu sub-spans of %u voices x %u buffers identical, %u images bit-exact, state restored\nPASS\n", spans, V, B, B);
        return 0;
    } catch (const std::exception &e) {
        printf("exception: %s\nFAIL\n", e.what());
        return 1;
    }
}
