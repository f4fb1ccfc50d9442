// sched_bank.hip -- event scheduling on the device: a voice bank is N independent instruments, each the scheduling half
// of Voice(T) (examples/example_song.zig:287-350: NoteTracker -> PolyphonyDispatcher(P) -> P Triggers), with the songs and
// all scheduler state resident in device memory.  One kernel advances every instrument by up to kBankChunk buffers and
// writes the [span][voice] tables the *_paint_spans entry points read: no host work per buffer beyond the launch, no
// host sync, no copy.  The per-lane steps are sched_lane.hip.h (the same text runs in a CPU harness); semantics are
// zh_poly_voice_schedule's (sched.hip), except for overflow (include/zang_hip.h).
//
// Shape: a workgroup owns `ipb` consecutive instruments (64 unless the polyphony makes their slots outgrow 64 KiB of LDS).
// Phase A, lane = instrument: consume the buffer's events and dispatch them; the dispatcher's slots live in LDS for the
// whole launch ([slot][instrument], so a wave's lanes hit different banks) and the result is a list of at most 32
// (slot, frame, event) entries per instrument, also in LDS.  Phase B, after a barrier, thread = sub-voice
// (instrument * P + slot): the Trigger loop over that slot's entries, writing row k of the tables -- adjacent threads
// are adjacent voices, so every store is a coalesced row segment.  Buffers loop A, B inside the launch.
#include "common.hip.h"
#include "sched_lane.hip.h"
#include "span_stage.hip.h"
#include <string.h>
#include <vector>

namespace {
constexpr uint32_t kBankBlock = 256, kBankChunk = 32, kBankMaxIpb = 64, kBankLdsBytes = 60 * 1024, kBankDefaultRows = 4,
                   kBankStageSlots = 4;

struct BankFrames { uint32_t n, base, first; uint32_t f[kBankChunk]; };   // by value: read when the call is made
struct BankArgs {
    ZsSong song;
    const uint32_t *offsets;                    // [n + 1]
    uint32_t n, P, ipb;
    // scheduler state
    uint32_t *next; float *t;                   // [n]
    uint32_t *slot_flags; uint64_t *slot_note, *slot_event;   // [n * P]
    uint32_t *trig_has, *trig_ev; uint64_t *trig_note;        // [n * P]
    // tables: rows of n * P voices; `plane` = capacity rows * voices (the distance between record words)
    uint32_t *count, *start, *end, *words;
    uint8_t *note_on, *changed;
    size_t plane;
    uint32_t max_spans;
    uint32_t *overflow;
};

static inline size_t bank_lds_bytes(uint32_t ipb, uint32_t P) { return (size_t)ipb * (3 * kZsMaxImpulses * 4 + 4 + (size_t)P * 20); }

__global__ void __launch_bounds__(kBankBlock) k_voice_bank_schedule(BankArgs a, BankFrames fr, float sample_rate) {
    extern __shared__ uint64_t bank_lds[];
    const uint32_t ipb = a.ipb, P = a.P, tid = threadIdx.x;
    uint64_t *s_note = bank_lds;                                  // [P][ipb]
    uint64_t *s_event = s_note + (size_t)P * ipb;                 // [P][ipb]
    uint32_t *s_flags = (uint32_t *)(s_event + (size_t)P * ipb);  // [P][ipb]
    uint32_t *l_slot = s_flags + (size_t)P * ipb;                 // [32][ipb]
    uint32_t *l_frame = l_slot + kZsMaxImpulses * ipb;
    uint32_t *l_ev = l_frame + kZsMaxImpulses * ipb;
    uint32_t *l_n = l_ev + kZsMaxImpulses * ipb;                  // [ipb]
    const uint32_t inst0 = blockIdx.x * ipb;
    const uint32_t n_inst = min(ipb, a.n - inst0);
    const uint32_t n_sub = n_inst * P;
    const size_t nv = (size_t)a.n * P, v0 = (size_t)inst0 * P;

    // slots of this workgroup's instruments: global [instrument][slot] -> LDS [slot][instrument], coalesced reads
    for (uint32_t j = tid; j < n_sub; j += kBankBlock) {
        const uint32_t li = (j % P) * ipb + j / P;
        s_flags[li] = a.slot_flags[v0 + j]; s_note[li] = a.slot_note[v0 + j]; s_event[li] = a.slot_event[v0 + j];
    }
    const bool lane_a = tid < n_inst;
    uint32_t next = 0, ev_begin = 0, ev_end = 0;
    float t = 0.0f;
    if (lane_a) { next = a.next[inst0 + tid]; t = a.t[inst0 + tid]; ev_begin = a.offsets[inst0 + tid]; ev_end = a.offsets[inst0 + tid + 1]; }
    __syncthreads();

    uint32_t dropped = 0, base = fr.base;
    for (uint32_t b = 0; b < fr.n; b++) {
        const uint32_t out_len = fr.f[b];
        if (lane_a) {                                                              // phase A
            const ZsSlots sl{s_flags + tid, s_note + tid, s_event + tid, ipb, P};
            const ZsList list{l_slot + tid, l_frame + tid, l_ev + tid, ipb};
            l_n[tid] = zs_consume_dispatch(a.song, ev_begin, ev_end, next, t, sample_rate, out_len, sl, list);
        }
        __syncthreads();
        for (uint32_t j = tid; j < n_sub; j += kBankBlock) {                       // phase B
            const uint32_t i = j / P, slot = j % P;
            const size_t v = v0 + j;
            const ZsList list{l_slot + i, l_frame + i, l_ev + i, ipb};
            ZsTrigger tr{a.trig_has[v], a.trig_ev[v], a.trig_note[v]};
            uint32_t k = (b == 0 && fr.first) ? 0u : a.count[v];
            zs_trigger_buffer(tr, a.song, list, l_n[i], slot, out_len, [&](uint32_t s, uint32_t e, uint32_t ev, uint32_t changed) {
                if (k >= a.max_spans) { dropped++; return; }
                const size_t idx = (size_t)k * nv + v;
                a.start[idx] = base + s; a.end[idx] = base + e;
                for (uint32_t w = 0; w < a.song.words; w++) a.words[w * a.plane + idx] = a.song.rec[(size_t)ev * a.song.words + w];
                a.note_on[idx] = zs_note_on(a.song, ev) ? 1 : 0;
                a.changed[idx] = (uint8_t)changed;
                k++;
            });
            a.count[v] = k;
            a.trig_has[v] = tr.has_note; a.trig_ev[v] = tr.ev; a.trig_note[v] = tr.note_id;
        }
        base += out_len;
        __syncthreads();
    }
    if (dropped) atomicAdd(a.overflow, dropped);
    if (lane_a) { a.next[inst0 + tid] = next; a.t[inst0 + tid] = t; }
    for (uint32_t j = tid; j < n_sub; j += kBankBlock) {
        const uint32_t li = (j % P) * ipb + j / P;
        a.slot_flags[v0 + j] = s_flags[li]; a.slot_note[v0 + j] = s_note[li]; a.slot_event[v0 + j] = s_event[li];
    }
}

// The live half: a bank with no song takes one batch of pushed impulses per buffer (ImpulseQueue -> PolyphonyDispatcher ->
// Trigger, examples/example_polyphony2.zig:61-95).  Same shape as above, one buffer per launch; the batch arrives sorted by
// instrument in CSR form, and a Trigger's carried note is its record, kept per voice in `carried` ([word][voice]).
struct LiveArgs {
    ZsSong batch;                               // note_id / rec of this call's impulses (t unused)
    const uint32_t *offsets, *frame;            // [n + 1], [impulses]
    uint32_t n, P, ipb;
    uint64_t *next_event_id;                    // [n]
    uint32_t *slot_flags; uint64_t *slot_note, *slot_event;   // [n * P]
    uint32_t *trig_has; uint64_t *trig_note;    // [n * P]
    uint32_t *carried;                          // [words][n * P]
    uint32_t *count, *start, *end, *words;
    uint8_t *note_on, *changed;
    size_t plane;
    uint32_t max_spans;
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kBankBlock) k_voice_bank_schedule_live(LiveArgs a, uint32_t out_len) {
    extern __shared__ uint64_t bank_lds[];
    const uint32_t ipb = a.ipb, P = a.P, tid = threadIdx.x;
    uint64_t *s_note = bank_lds;                                  // [P][ipb]
    uint64_t *s_event = s_note + (size_t)P * ipb;                 // [P][ipb]
    uint32_t *s_flags = (uint32_t *)(s_event + (size_t)P * ipb);  // [P][ipb]
    uint32_t *l_slot = s_flags + (size_t)P * ipb;                 // [32][ipb]
    uint32_t *l_frame = l_slot + kZsMaxImpulses * ipb;
    uint32_t *l_ev = l_frame + kZsMaxImpulses * ipb;
    uint32_t *l_n = l_ev + kZsMaxImpulses * ipb;                  // [ipb]
    const uint32_t inst0 = blockIdx.x * ipb;
    const uint32_t n_inst = min(ipb, a.n - inst0);
    const uint32_t n_sub = n_inst * P;
    const size_t nv = (size_t)a.n * P, v0 = (size_t)inst0 * P;

    for (uint32_t j = tid; j < n_sub; j += kBankBlock) {
        const uint32_t li = (j % P) * ipb + j / P;
        s_flags[li] = a.slot_flags[v0 + j]; s_note[li] = a.slot_note[v0 + j]; s_event[li] = a.slot_event[v0 + j];
    }
    __syncthreads();
    if (tid < n_inst) {                                                            // phase A
        const ZsSlots sl{s_flags + tid, s_note + tid, s_event + tid, ipb, P};
        const ZsList list{l_slot + tid, l_frame + tid, l_ev + tid, ipb};
        uint64_t next_id = a.next_event_id[inst0 + tid];
        l_n[tid] = zs_push_dispatch(a.batch, a.frame, a.offsets[inst0 + tid], a.offsets[inst0 + tid + 1], next_id, sl, list);
        a.next_event_id[inst0 + tid] = next_id;
    }
    __syncthreads();
    uint32_t dropped = 0;
    for (uint32_t j = tid; j < n_sub; j += kBankBlock) {                           // phase B
        const uint32_t i = j / P, slot = j % P;
        const size_t v = v0 + j;
        const ZsList list{l_slot + i, l_frame + i, l_ev + i, ipb};
        const ZsCarried carried{a.carried + v, nv};
        ZsTrigger tr{a.trig_has[v], kZsCarried, a.trig_note[v]};
        uint32_t k = 0;
        zs_trigger_buffer(tr, a.batch, list, l_n[i], slot, out_len, [&](uint32_t s, uint32_t e, uint32_t ev, uint32_t changed) {
            if (k >= a.max_spans) { dropped++; return; }
            const size_t idx = (size_t)k * nv + v;
            a.start[idx] = s; a.end[idx] = e;
            for (uint32_t w = 0; w < a.batch.words; w++) a.words[w * a.plane + idx] = zs_live_word(a.batch, carried, ev, w);
            a.note_on[idx] = zs_live_note_on(a.batch, carried, ev) ? 1 : 0;
            a.changed[idx] = (uint8_t)changed;
            k++;
        });
        zs_live_keep(tr, a.batch, carried);
        a.count[v] = k;
        a.trig_has[v] = tr.has_note; a.trig_note[v] = tr.note_id;
    }
    if (dropped) atomicAdd(a.overflow, dropped);
    for (uint32_t j = tid; j < n_sub; j += kBankBlock) {
        const uint32_t li = (j % P) * ipb + j / P;
        a.slot_flags[v0 + j] = s_flags[li]; a.slot_note[v0 + j] = s_note[li]; a.slot_event[v0 + j] = s_event[li];
    }
}
}  // namespace

struct zh_voice_bank : zh_stage {                 // tab: rows of n * P voices, one field per record word
    uint32_t n, P, words, note_on_offset, ipb;
    uint64_t n_events;
    float *t; uint64_t *note_id; uint32_t *rec, *offsets;
    uint32_t *next; float *clock;
    uint32_t *slot_flags, *trig_has, *trig_ev; uint64_t *slot_note, *slot_event, *trig_note;
    uint8_t *note_on;                             // [rows][n * P], beside the table's rows
    // a live bank (zh_voice_bank_create_live): no song, no tracker; per call one batch of pushed impulses
    bool live;
    uint32_t max_impulses;
    uint64_t *next_event_id;                      // [n] ImpulseQueue.next_event_id
    uint32_t *carried;                            // [words][n * P] the Triggers' carried records
    uint8_t *batch;                               // device copy of the call's sorted batch (bank_batch_bytes at most)
    uint8_t *stage[kBankStageSlots];              // pinned host staging, a ring: slot k is free once stage_done[k] has passed
    hipEvent_t stage_done[kBankStageSlots];
    uint32_t stage_next;
};

namespace {
// a batch of m impulses as ONE block: u64 note_id[m], u32 offsets[n + 1], u32 frame[m], u32 rec[m][words]
size_t bank_batch_bytes(const zh_voice_bank *b, size_t m) { return m * 8 + ((size_t)b->n + 1) * 4 + m * 4 + m * 4 * b->words; }
size_t bank_voices(const zh_voice_bank *b) { return (size_t)b->n * b->P; }
void bank_free(zh_voice_bank *b) {
    stage_free(b->tab);
    (void)hipFree(b->note_on);
    (void)hipFree(b->t); (void)hipFree(b->note_id); (void)hipFree(b->rec); (void)hipFree(b->offsets); (void)hipFree(b->next); (void)hipFree(b->clock);
    (void)hipFree(b->slot_flags); (void)hipFree(b->trig_has); (void)hipFree(b->trig_ev); (void)hipFree(b->slot_note); (void)hipFree(b->slot_event);
    (void)hipFree(b->trig_note);
    (void)hipFree(b->next_event_id); (void)hipFree(b->carried); (void)hipFree(b->batch);
    for (uint32_t k = 0; k < kBankStageSlots; k++) {
        if (b->stage[k]) (void)hipHostFree(b->stage[k]);
        if (b->stage_done[k]) (void)hipEventDestroy(b->stage_done[k]);
    }
}
// the table with kBankDefaultRows rows and the note_on plane beside it
int bank_create_tables(zh_voice_bank *b) {
    int rc = stage_create(b, (uint32_t)bank_voices(b), b->words, kBankDefaultRows);
    if (!rc) rc = dev_alloc(&b->note_on, kBankDefaultRows * bank_voices(b));
    return rc;
}
int bank_clear_state(zh_voice_bank *b) {                          // example_song.zig:318-324 (and Trigger.init / NoteTracker.init)
    const size_t nv = bank_voices(b);
    hipStream_t st = b->ctx->stream;
    // (a live bank has no tracker, and ImpulseQueue has no reset: next_event_id stays)
    if (b->n && !b->live) { ZH_TRY(hipMemsetAsync(b->next, 0, (size_t)b->n * 4, st)); ZH_TRY(hipMemsetAsync(b->clock, 0, (size_t)b->n * 4, st)); }
    if (nv) {
        ZH_TRY(hipMemsetAsync(b->slot_flags, 0, nv * 4, st)); ZH_TRY(hipMemsetAsync(b->slot_note, 0, nv * 8, st));
        ZH_TRY(hipMemsetAsync(b->slot_event, 0, nv * 8, st)); ZH_TRY(hipMemsetAsync(b->trig_has, 0, nv * 4, st));
        ZH_TRY(hipMemsetAsync(b->trig_note, 0, nv * 8, st));
        if (!b->live) ZH_TRY(hipMemsetAsync(b->trig_ev, 0, nv * 4, st));
    }
    return ZH_OK;
}
template <typename T> int bank_down(zh_voice_bank *b, std::vector<T> &h, const T *d, size_t n) {
    h.resize(n);
    return n ? zh_download(b->ctx, h.data(), d, n * sizeof(T)) : ZH_OK;
}
}  // namespace

extern "C" {

int zh_voice_bank_create(zh_ctx *ctx, uint32_t n_instruments, uint32_t polyphony, uint32_t params_size, uint32_t note_on_offset,
                         const uint64_t *event_offsets, const void *paramses, const float *t, const uint64_t *note_ids, zh_voice_bank **out) {
    ZH_GUARD(ctx);
    if (!ctx || !out || polyphony == 0 || params_size == 0 || params_size > ZH_MAX_PARAMS_SIZE || (params_size & 3u) ||
        note_on_offset >= params_size || (n_instruments && !event_offsets))
        return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    uint64_t n_events = 0;
    for (uint32_t i = 0; i < n_instruments; i++) if (event_offsets[i + 1] < event_offsets[i]) return ZH_ERR_INVALID;
    if (n_instruments) { if (event_offsets[0] != 0) return ZH_ERR_INVALID; n_events = event_offsets[n_instruments]; }
    if (n_events >= 0xffffffffull || (n_events && (!paramses || !t || !note_ids))) return ZH_ERR_INVALID;
    if ((uint64_t)n_instruments * polyphony > (1ull << 31)) return ZH_ERR_INVALID;
    uint32_t ipb = kBankMaxIpb;
    while (ipb > 1 && bank_lds_bytes(ipb, polyphony) > kBankLdsBytes) ipb /= 2;
    if (bank_lds_bytes(ipb, polyphony) > kBankLdsBytes) return ZH_ERR_INVALID;     // (a polyphony of about 3,000)
    zh_voice_bank *b = new (std::nothrow) zh_voice_bank();
    if (!b) return ZH_ERR_INVALID;
    memset(b, 0, sizeof *b);
    b->ctx = ctx; b->n = n_instruments; b->P = polyphony; b->words = params_size / 4; b->note_on_offset = note_on_offset; b->ipb = ipb;
    b->n_events = n_events;
    const size_t nv = bank_voices(b);
    int rc = dev_alloc(&b->t, n_events);
    if (!rc) rc = dev_alloc(&b->note_id, n_events);
    if (!rc) rc = dev_alloc(&b->rec, n_events * b->words);
    if (!rc) rc = dev_alloc(&b->offsets, n_instruments ? (size_t)n_instruments + 1 : 0);
    if (!rc) rc = dev_alloc(&b->next, n_instruments);
    if (!rc) rc = dev_alloc(&b->clock, n_instruments);
    if (!rc) rc = dev_alloc(&b->slot_flags, nv);
    if (!rc) rc = dev_alloc(&b->slot_note, nv);
    if (!rc) rc = dev_alloc(&b->slot_event, nv);
    if (!rc) rc = dev_alloc(&b->trig_has, nv);
    if (!rc) rc = dev_alloc(&b->trig_ev, nv);
    if (!rc) rc = dev_alloc(&b->trig_note, nv);
    if (!rc) rc = bank_create_tables(b);
    if (!rc) rc = bank_clear_state(b);
    if (!rc && n_events) {
        rc = zh_upload(ctx, b->t, t, n_events * 4);
        if (!rc) rc = zh_upload(ctx, b->note_id, note_ids, n_events * 8);
        if (!rc) rc = zh_upload(ctx, b->rec, paramses, n_events * params_size);
    }
    if (!rc && n_instruments) {
        std::vector<uint32_t> off((size_t)n_instruments + 1);
        for (uint32_t i = 0; i <= n_instruments; i++) off[i] = (uint32_t)event_offsets[i];
        rc = zh_upload(ctx, b->offsets, off.data(), off.size() * 4);
    }
    if (rc) return stage_create_failed(b, bank_free, rc);
    *out = b;
    return ZH_OK;
}

int zh_voice_bank_destroy(zh_voice_bank *b) { ZH_GUARD(b ? b->ctx : nullptr); return stage_destroy(b, bank_free); }

int zh_voice_bank_reset(zh_voice_bank *b) { ZH_GUARD(b ? b->ctx : nullptr);
    if (!b) return ZH_ERR_INVALID;
    return bank_clear_state(b);
}

int zh_voice_bank_reserve(zh_voice_bank *b, uint32_t max_rows) { ZH_GUARD(b ? b->ctx : nullptr);
    const uint32_t had = b ? b->tab.rows : 0;
    int rc = stage_reserve(b, max_rows);
    if (rc || b->tab.rows == had) return rc;                      // refused, or the same capacity
    (void)hipFree(b->note_on);                                    // (the stream is idle: stage_reserve)
    rc = dev_alloc(&b->note_on, (size_t)max_rows * bank_voices(b));
    if (rc) { stage_free_rows(b->tab); (void)hipGetLastError(); }
    return rc;
}

int zh_voice_bank_schedule(zh_voice_bank *b, float sample_rate, const uint32_t *frames, uint32_t n_buffers, uint32_t max_spans) {
    ZH_GUARD(b ? b->ctx : nullptr);
    if (!stage_spans_ok(b, max_spans) || b->live || (n_buffers && !frames)) return ZH_ERR_INVALID;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_buffers; i++) total += frames[i];
    if (total >> 32) return ZH_ERR_INVALID;
    if (b->n == 0) return ZH_OK;
    hipStream_t st = b->ctx->stream;
    const StageRows rows = stage_rows(b);
    if (n_buffers == 0) { ZH_TRY(hipMemsetAsync(rows.count, 0, bank_voices(b) * 4, st)); return ZH_OK; }
    BankArgs a;
    a.song = ZsSong{b->t, b->note_id, b->rec, b->words, b->note_on_offset / 4, (b->note_on_offset & 3u) * 8};
    a.offsets = b->offsets; a.n = b->n; a.P = b->P; a.ipb = b->ipb;
    a.next = b->next; a.t = b->clock;
    a.slot_flags = b->slot_flags; a.slot_note = b->slot_note; a.slot_event = b->slot_event;
    a.trig_has = b->trig_has; a.trig_ev = b->trig_ev; a.trig_note = b->trig_note;
    a.count = rows.count; a.start = rows.start; a.end = rows.end; a.words = rows.words; a.note_on = b->note_on; a.changed = rows.changed;
    a.plane = rows.plane; a.max_spans = max_spans; a.overflow = b->tab.overflow;
    const dim3 grid((b->n + b->ipb - 1) / b->ipb);
    const size_t lds = bank_lds_bytes(b->ipb, b->P);
    BankFrames fr;
    fr.base = 0;
    for (uint32_t done = 0; done < n_buffers; done += kBankChunk) {
        fr.n = n_buffers - done < kBankChunk ? n_buffers - done : kBankChunk;
        fr.first = done == 0;
        for (uint32_t i = 0; i < kBankChunk; i++) fr.f[i] = i < fr.n ? frames[done + i] : 0u;
        ZH_LAUNCH(k_voice_bank_schedule, grid, dim3(kBankBlock), lds, st, a, fr, sample_rate);
        for (uint32_t i = 0; i < fr.n; i++) fr.base += fr.f[i];
    }
    return zh_launch_status();
}

int zh_voice_bank_script_table(const zh_voice_bank *b, uint32_t max_spans, zh_script_span_table *out) { return stage_script_table(b, max_spans, out); }
int zh_voice_bank_span_param(const zh_voice_bank *b, uint32_t word, zh_script_span_param *out) { return stage_span_param(b, word, 0, out); }
int zh_voice_bank_span_table(const zh_voice_bank *b, uint32_t max_spans, uint32_t freq_word, zh_span_table *out) {
    zh_script_span_table t;
    zh_script_span_param freq;
    if (!out || stage_script_table(b, max_spans, &t) || stage_span_param(b, freq_word, 'f', &freq)) return ZH_ERR_INVALID;
    *out = zh_span_table{max_spans, 0, t.count, t.start, t.end, freq.f, b->note_on, t.note_id_changed};
    return ZH_OK;
}
int zh_voice_bank_overflows(zh_voice_bank *b, uint64_t *out) { ZH_GUARD(b ? b->ctx : nullptr); return stage_overflows(b, out); }

int zh_voice_bank_get_state(zh_voice_bank *b, zh_voice_bank_instrument_state *instruments, zh_voice_bank_voice_state *voices) {
    ZH_GUARD(b ? b->ctx : nullptr);
    if (!b || b->live || (b->n && (!instruments || !voices))) return ZH_ERR_INVALID;
    const size_t nv = bank_voices(b);
    std::vector<uint32_t> next, sf, th, te;
    std::vector<float> clock;
    std::vector<uint64_t> sn, se, tn;
    int rc = bank_down(b, next, b->next, b->n);
    if (!rc) rc = bank_down(b, clock, b->clock, b->n);
    if (!rc) rc = bank_down(b, sf, b->slot_flags, nv);
    if (!rc) rc = bank_down(b, sn, b->slot_note, nv);
    if (!rc) rc = bank_down(b, se, b->slot_event, nv);
    if (!rc) rc = bank_down(b, th, b->trig_has, nv);
    if (!rc) rc = bank_down(b, te, b->trig_ev, nv);
    if (!rc) rc = bank_down(b, tn, b->trig_note, nv);
    if (rc) return rc;
    for (uint32_t i = 0; i < b->n; i++) instruments[i] = zh_voice_bank_instrument_state{next[i], clock[i], 0};
    for (size_t v = 0; v < nv; v++)
        voices[v] = zh_voice_bank_voice_state{(sf[v] & ZS_SLOT_USED) ? 1u : 0u, (sf[v] & ZS_SLOT_ON) ? 1u : 0u, sn[v], se[v], th[v] ? 1u : 0u, 0, tn[v], te[v]};
    return ZH_OK;
}

int zh_voice_bank_set_state(zh_voice_bank *b, const zh_voice_bank_instrument_state *instruments, const zh_voice_bank_voice_state *voices) {
    ZH_GUARD(b ? b->ctx : nullptr);
    if (!b || b->live || (b->n && (!instruments || !voices))) return ZH_ERR_INVALID;
    if (b->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    const size_t nv = bank_voices(b);
    if (!nv) return ZH_OK;
    std::vector<uint32_t> next(b->n), sf(nv), th(nv), te(nv);
    std::vector<float> clock(b->n);
    std::vector<uint64_t> sn(nv), se(nv), tn(nv);
    for (uint32_t i = 0; i < b->n; i++) {
        if (instruments[i].next_event > 0xffffffffull) return ZH_ERR_INVALID;
        next[i] = (uint32_t)instruments[i].next_event; clock[i] = instruments[i].t;
    }
    for (size_t v = 0; v < nv; v++) {
        if (voices[v].has_note && voices[v].trigger_event >= b->n_events) return ZH_ERR_INVALID;   // the kernel reads the song at it
        sf[v] = (voices[v].used ? ZS_SLOT_USED : 0u) | (voices[v].note_on ? ZS_SLOT_ON : 0u);
        sn[v] = voices[v].note_id; se[v] = voices[v].event_id;
        th[v] = voices[v].has_note ? 1u : 0u; te[v] = voices[v].has_note ? (uint32_t)voices[v].trigger_event : 0u; tn[v] = voices[v].trigger_note_id;
    }
    int rc = zh_upload(b->ctx, b->next, next.data(), (size_t)b->n * 4);
    if (!rc) rc = zh_upload(b->ctx, b->clock, clock.data(), (size_t)b->n * 4);
    if (!rc) rc = zh_upload(b->ctx, b->slot_flags, sf.data(), nv * 4);
    if (!rc) rc = zh_upload(b->ctx, b->slot_note, sn.data(), nv * 8);
    if (!rc) rc = zh_upload(b->ctx, b->slot_event, se.data(), nv * 8);
    if (!rc) rc = zh_upload(b->ctx, b->trig_has, th.data(), nv * 4);
    if (!rc) rc = zh_upload(b->ctx, b->trig_ev, te.data(), nv * 4);
    if (!rc) rc = zh_upload(b->ctx, b->trig_note, tn.data(), nv * 8);
    return rc;
}

int zh_voice_bank_create_live(zh_ctx *ctx, uint32_t n_instruments, uint32_t polyphony, uint32_t params_size, uint32_t note_on_offset,
                              uint32_t max_impulses_per_call, zh_voice_bank **out) {
    ZH_GUARD(ctx);
    if (!ctx || !out || polyphony == 0 || params_size == 0 || params_size > ZH_MAX_PARAMS_SIZE || (params_size & 3u) ||
        note_on_offset >= params_size || max_impulses_per_call == kZsCarried)
        return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    if ((uint64_t)n_instruments * polyphony > (1ull << 31)) return ZH_ERR_INVALID;
    uint32_t ipb = kBankMaxIpb;
    while (ipb > 1 && bank_lds_bytes(ipb, polyphony) > kBankLdsBytes) ipb /= 2;
    if (bank_lds_bytes(ipb, polyphony) > kBankLdsBytes) return ZH_ERR_INVALID;
    zh_voice_bank *b = new (std::nothrow) zh_voice_bank();
    if (!b) return ZH_ERR_INVALID;
    memset(b, 0, sizeof *b);
    b->ctx = ctx; b->n = n_instruments; b->P = polyphony; b->words = params_size / 4; b->note_on_offset = note_on_offset; b->ipb = ipb;
    b->live = true; b->max_impulses = max_impulses_per_call;
    const size_t nv = bank_voices(b), bytes = bank_batch_bytes(b, max_impulses_per_call);
    int rc = dev_alloc(&b->next_event_id, n_instruments);
    if (!rc) rc = dev_alloc(&b->slot_flags, nv);
    if (!rc) rc = dev_alloc(&b->slot_note, nv);
    if (!rc) rc = dev_alloc(&b->slot_event, nv);
    if (!rc) rc = dev_alloc(&b->trig_has, nv);
    if (!rc) rc = dev_alloc(&b->trig_note, nv);
    if (!rc) rc = dev_alloc(&b->carried, nv * b->words);
    if (!rc && n_instruments) rc = dev_alloc(&b->batch, bytes);
    for (uint32_t k = 0; !rc && n_instruments && k < kBankStageSlots; k++) {
        rc = (int)hipHostMalloc((void **)&b->stage[k], bytes, hipHostMallocDefault);
        if (!rc) rc = (int)hipEventCreateWithFlags(&b->stage_done[k], hipEventDisableTiming);
    }
    if (!rc) rc = bank_create_tables(b);
    if (!rc && nv) rc = (int)hipMemsetAsync(b->carried, 0, nv * b->words * 4, ctx->stream);
    if (!rc) rc = bank_clear_state(b);
    if (!rc && n_instruments) {                                                    // ImpulseQueue.init: next_event_id = 1
        const std::vector<uint64_t> ones(n_instruments, 1);
        rc = zh_upload(ctx, b->next_event_id, ones.data(), (size_t)n_instruments * 8);
    }
    if (rc) return stage_create_failed(b, bank_free, rc);
    *out = b;
    return ZH_OK;
}

int zh_voice_bank_schedule_live(zh_voice_bank *b, uint32_t out_len, uint32_t max_spans, const zh_bank_impulses *batch) {
    ZH_GUARD(b ? b->ctx : nullptr);
    if (!stage_spans_ok(b, max_spans) || !b->live) return ZH_ERR_INVALID;
    const uint32_t m = batch ? batch->n : 0u;
    if (m > b->max_impulses || (m && (!batch->instrument || !batch->frame || !batch->note_id || !batch->paramses))) return ZH_ERR_INVALID;
    for (uint32_t i = 0; i < m; i++) if (batch->instrument[i] >= b->n) return ZH_ERR_INVALID;
    if (b->ctx->capturing) return ZH_ERR_UNSUPPORTED;             // (a replay would read host memory that has since changed)
    if (b->n == 0) return ZH_OK;
    hipStream_t st = b->ctx->stream;
    // the batch, sorted by instrument (a stable counting sort into CSR), in a staging slot whose last copy has completed
    const uint32_t slot = b->stage_next;
    b->stage_next = (slot + 1) % kBankStageSlots;
    ZH_TRY(hipEventSynchronize(b->stage_done[slot]));
    uint8_t *h = b->stage[slot];
    uint64_t *h_note = (uint64_t *)h;
    uint32_t *h_off = (uint32_t *)(h + (size_t)m * 8), *h_frame = h_off + b->n + 1, *h_rec = h_frame + m;
    memset(h_off, 0, ((size_t)b->n + 1) * 4);
    for (uint32_t i = 0; i < m; i++) h_off[batch->instrument[i] + 1] += 1;
    for (uint32_t i = 0; i < b->n; i++) h_off[i + 1] += h_off[i];
    const size_t psize = (size_t)b->words * 4;
    for (uint32_t i = 0; i < m; i++) {                            // h_off[k] = the next free place of instrument k ...
        const uint32_t at = h_off[batch->instrument[i]]++;
        h_note[at] = batch->note_id[i]; h_frame[at] = batch->frame[i];
        memcpy(h_rec + (size_t)at * b->words, (const uint8_t *)batch->paramses + i * psize, psize);
    }
    for (uint32_t i = b->n; i > 0; i--) h_off[i] = h_off[i - 1];  // ... = the begin of k + 1 once all are placed: shift back
    h_off[0] = 0;
    ZH_TRY(hipMemcpyAsync(b->batch, h, bank_batch_bytes(b, m), hipMemcpyHostToDevice, st));
    ZH_TRY(hipEventRecord(b->stage_done[slot], st));
    LiveArgs a;
    uint8_t *d = b->batch;
    a.batch = ZsSong{nullptr, (const uint64_t *)d, (const uint32_t *)(d + (size_t)m * 8) + b->n + 1 + m, b->words, b->note_on_offset / 4,
                     (b->note_on_offset & 3u) * 8};
    a.offsets = (const uint32_t *)(d + (size_t)m * 8); a.frame = a.offsets + b->n + 1;
    a.n = b->n; a.P = b->P; a.ipb = b->ipb;
    a.next_event_id = b->next_event_id;
    a.slot_flags = b->slot_flags; a.slot_note = b->slot_note; a.slot_event = b->slot_event;
    a.trig_has = b->trig_has; a.trig_note = b->trig_note; a.carried = b->carried;
    const StageRows rows = stage_rows(b);
    a.count = rows.count; a.start = rows.start; a.end = rows.end; a.words = rows.words; a.note_on = b->note_on; a.changed = rows.changed;
    a.plane = rows.plane; a.max_spans = max_spans; a.overflow = b->tab.overflow;
    ZH_LAUNCH(k_voice_bank_schedule_live, dim3((b->n + b->ipb - 1) / b->ipb), dim3(kBankBlock), bank_lds_bytes(b->ipb, b->P), st, a, out_len);
    return zh_launch_status();
}

int zh_voice_bank_live_get_state(zh_voice_bank *b, uint64_t *next_event_id, zh_voice_bank_live_voice_state *voices) {
    ZH_GUARD(b ? b->ctx : nullptr);
    if (!b || !b->live || (b->n && (!next_event_id || !voices))) return ZH_ERR_INVALID;
    const size_t nv = bank_voices(b);
    std::vector<uint32_t> sf, th, cw;
    std::vector<uint64_t> sn, se, tn;
    int rc = b->n ? zh_download(b->ctx, next_event_id, b->next_event_id, (size_t)b->n * 8) : ZH_OK;
    if (!rc) rc = bank_down(b, sf, b->slot_flags, nv);
    if (!rc) rc = bank_down(b, sn, b->slot_note, nv);
    if (!rc) rc = bank_down(b, se, b->slot_event, nv);
    if (!rc) rc = bank_down(b, th, b->trig_has, nv);
    if (!rc) rc = bank_down(b, tn, b->trig_note, nv);
    if (!rc) rc = bank_down(b, cw, b->carried, nv * b->words);
    if (rc) return rc;
    for (size_t v = 0; v < nv; v++) {
        zh_voice_bank_live_voice_state s;
        memset(&s, 0, sizeof s);
        s.used = (sf[v] & ZS_SLOT_USED) ? 1u : 0u; s.note_on = (sf[v] & ZS_SLOT_ON) ? 1u : 0u; s.note_id = sn[v]; s.event_id = se[v];
        s.has_note = th[v] ? 1u : 0u; s.trigger_note_id = tn[v];
        if (s.has_note) for (uint32_t w = 0; w < b->words; w++) s.carried[w] = cw[w * nv + v];
        voices[v] = s;
    }
    return ZH_OK;
}

int zh_voice_bank_live_set_state(zh_voice_bank *b, const uint64_t *next_event_id, const zh_voice_bank_live_voice_state *voices) {
    ZH_GUARD(b ? b->ctx : nullptr);
    if (!b || !b->live || (b->n && (!next_event_id || !voices))) return ZH_ERR_INVALID;
    if (b->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    const size_t nv = bank_voices(b);
    if (!nv) return ZH_OK;
    std::vector<uint32_t> sf(nv), th(nv), cw(nv * b->words);
    std::vector<uint64_t> sn(nv), se(nv), tn(nv);
    for (size_t v = 0; v < nv; v++) {
        sf[v] = (voices[v].used ? ZS_SLOT_USED : 0u) | (voices[v].note_on ? ZS_SLOT_ON : 0u);
        sn[v] = voices[v].note_id; se[v] = voices[v].event_id;
        th[v] = voices[v].has_note ? 1u : 0u; tn[v] = voices[v].trigger_note_id;
        for (uint32_t w = 0; w < b->words; w++) cw[w * nv + v] = voices[v].carried[w];
    }
    int rc = zh_upload(b->ctx, b->next_event_id, next_event_id, (size_t)b->n * 8);
    if (!rc) rc = zh_upload(b->ctx, b->slot_flags, sf.data(), nv * 4);
    if (!rc) rc = zh_upload(b->ctx, b->slot_note, sn.data(), nv * 8);
    if (!rc) rc = zh_upload(b->ctx, b->slot_event, se.data(), nv * 8);
    if (!rc) rc = zh_upload(b->ctx, b->trig_has, th.data(), nv * 4);
    if (!rc) rc = zh_upload(b->ctx, b->trig_note, tn.data(), nv * 8);
    if (!rc) rc = zh_upload(b->ctx, b->carried, cw.data(), nv * b->words * 4);
    return rc;
}

}  // extern "C"
