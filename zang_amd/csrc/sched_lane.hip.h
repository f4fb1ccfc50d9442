// sched_lane.hip.h -- the per-lane steps of the voice bank's scheduling kernel (sched_bank.hip), written once as
// __host__ __device__ functions so that the same text runs in a CPU harness (tests/cpp/sched_lane_host.cpp).
// Semantics are those of zh_poly_voice_schedule (sched.hip: notes.zig:138-207, 209-349, trigger.zig:26-198), what that
// file defines where the reference is undefined included.  What differs is the data: params never move.  An impulse is
// (slot, frame, index of its song event); a Trigger's carried note is an event index; record words and note ids are
// read from the song by that index.  An instrument's event_id is its event's position in the instrument's song + 1.
// Events of a bank are indexed with 32 bits (fewer than 2^32 - 1 of them), frames of one buffer too.
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZS_HD __host__ __device__ inline
#else
#define ZS_HD inline
#endif

constexpr uint32_t kZsMaxImpulses = 32;     // ZH_MAX_IMPULSES (notes.zig:73-74)

// The songs of a bank in CSR form: instrument i owns events [offsets[i], offsets[i + 1]) of the shared arrays.
struct ZsSong {
    const float *t;            // [events] seconds
    const uint64_t *note_id;   // [events]
    const uint32_t *rec;       // [events][words] the params records, as 32-bit words
    uint32_t words;            // params_size / 4
    uint32_t on_word, on_shift;   // note_on is byte (on_shift / 8) of word on_word
};
ZS_HD bool zs_note_on(const ZsSong &s, uint32_t ev) { return ((s.rec[(size_t)ev * s.words + s.on_word] >> s.on_shift) & 0xffu) != 0; }

// PolyphonyDispatcher's slots of ONE instrument: slot s lives at index s * stride (stride 1 on the host, the number of
// instruments per workgroup in LDS, so that the lanes of a wave hit different banks).
struct ZsSlots {
    uint32_t *flags;           // bit 0 used, bit 1 note_on
    uint64_t *note_id, *event_id;
    uint32_t stride, polyphony;
};
enum { ZS_SLOT_USED = 1u, ZS_SLOT_ON = 2u };
// The impulses one buffer delivers to ONE instrument, in order: entry i at index i * stride.
struct ZsList {
    uint32_t *slot, *frame, *ev;
    uint32_t stride;
};
// Trigger's state between buffers: "once set, never set back to null" (trigger.zig:39-41)
struct ZsTrigger { uint32_t has_note, ev; uint64_t note_id; };

// chooseSlot, notes.zig:246-306; -1 for null
ZS_HD int32_t zs_choose_slot(const ZsSlots &sl, uint64_t note_id, bool note_on) {
    const uint32_t P = sl.polyphony, st = sl.stride;
    if (!note_on) {                                                                   // :253-264
        for (uint32_t i = 0; i < P; i++)
            if (sl.flags[i * st] == (ZS_SLOT_USED | ZS_SLOT_ON) && sl.note_id[i * st] == note_id) return (int32_t)i;
        return -1;
    }
    int32_t best = -1;                                                                // :269-293
    uint64_t best_id = 0;
    for (uint32_t i = 0; i < P; i++) {
        const uint32_t f = sl.flags[i * st];
        if (!(f & ZS_SLOT_USED)) return (int32_t)i;                                   // empty slot: take it now
        if (!(f & ZS_SLOT_ON)) {
            const uint64_t e = sl.event_id[i * st];
            if (best < 0 || e < best_id) { best = (int32_t)i; best_id = e; }
        }
    }
    if (best >= 0) return best;
    uint32_t b = 0;                                                                   // :296-305 steal the stalest note-on
    uint64_t b_id = sl.event_id[0];
    for (uint32_t i = 1; i < P; i++) {
        const uint64_t e = sl.event_id[i * st];
        if (e < b_id) { b = i; b_id = e; }
    }
    return (int32_t)b;
}

// One impulse through PolyphonyDispatcher.dispatch (notes.zig:316-336): choose its slot, update the slot, list it.
// `listed` = entries so far; returns the new number (an impulse no slot takes is not listed).
ZS_HD uint32_t zs_dispatch_one(const ZsSlots &sl, const ZsList &list, uint32_t listed, uint32_t frame, uint32_t ev, uint64_t note_id,
                               bool on, uint64_t event_id) {
    const int32_t slot = zs_choose_slot(sl, note_id, on);
    if (slot < 0) return listed;
    const uint32_t si = (uint32_t)slot * sl.stride;
    sl.flags[si] = ZS_SLOT_USED | (on ? ZS_SLOT_ON : 0u);
    sl.note_id[si] = note_id;
    sl.event_id[si] = event_id;
    const uint32_t li = listed * list.stride;
    list.slot[li] = (uint32_t)slot; list.frame[li] = frame; list.ev[li] = ev;
    return listed + 1;
}

// NoteTracker.consume (notes.zig:160-206) of one buffer of out_len frames, each impulse handed straight to the dispatcher
// (which does not feed back into the tracker, so one pass is the two calls).  `next` counts from the instrument's first
// event.  Returns the number of list entries (at most 32: a 33rd impulse is dropped while `next` still advances).
ZS_HD uint32_t zs_consume_dispatch(const ZsSong &song, uint32_t ev_begin, uint32_t ev_end, uint32_t &next, float &t, float sample_rate,
                                   uint32_t out_len, const ZsSlots &sl, const ZsList &list) {
    uint32_t count = 0, listed = 0;
    const float buf_time = (float)out_len / sample_rate;                              // :170
    const float end_t = t + buf_time;                                                 // :172
    const uint64_t last = (uint64_t)out_len - 1;
    const uint32_t n = ev_end - ev_begin;
    while (next < n) {
        const uint32_t ev = ev_begin + next;
        const float note_t = song.t[ev];
        if (!(note_t < end_t)) break;                                                 // :178, :195-197
        const float f = (note_t - t) / buf_time;                                      // :179
        const float pos = f * (float)out_len;
        uint64_t rel = 0;
        if (pos == pos && pos > 0.0f) rel = pos >= 1.8446744073709552e19f ? ~0ull : (uint64_t)pos;
        if (rel > last) rel = last;                                                   // :180-183
        next += 1;                                                                    // :186
        if (count < kZsMaxImpulses) {                                                 // :187-191; event_id = next
            count += 1;
            listed = zs_dispatch_one(sl, list, listed, (uint32_t)rel, ev, song.note_id[ev], zs_note_on(song, ev), (uint64_t)next);
        }
    }
    t = end_t;                                                                        // :200
    return listed;
}

// the next entry at or after `from` that went to `slot` (n = none)
ZS_HD uint32_t zs_next_of(const ZsList &list, uint32_t n, uint32_t slot, uint32_t from) {
    while (from < n && list.slot[from * list.stride] != slot) from++;
    return from;
}

// Trigger.counter + the Trigger.next loop (trigger.zig:66-196) of one sub-voice over one buffer: emit(start, end, ev,
// note_id_changed) for every sub-span that holds a note, in order.  `ev` is the event whose record the paint takes.
template <class Emit>
ZS_HD void zs_trigger_buffer(ZsTrigger &tr, const ZsSong &song, const ZsList &list, uint32_t n, uint32_t slot, uint32_t out_len, Emit &&emit) {
    uint32_t start = 0;
    const uint32_t end = out_len;
    uint32_t cur = zs_next_of(list, n, slot, 0);                                      // impulse_index
    while (start < end) {
        bool has = false, found = false;
        uint32_t s_end = end, ev = 0;
        uint64_t id = 0;
        if (tr.has_note) {                                                            // carryOver :107-137
            if (cur < n) {
                const uint32_t nf = list.frame[cur * list.stride];
                if (nf > start) { s_end = nf < end ? nf : end; found = true; }
            } else found = true;
            if (found) { has = true; ev = tr.ev; id = tr.note_id; }
        }
        if (!found) {                                                                 // getNextNoteSpan :139-196
            while (cur < n) {
                const uint32_t f = list.frame[cur * list.stride];
                if (f >= end) break;
                if (f > start) { s_end = f; break; }
                const uint32_t this_ev = list.ev[cur * list.stride];
                cur = zs_next_of(list, n, slot, cur + 1);
                uint32_t clipped = end;
                if (cur < n) { const uint32_t nf = list.frame[cur * list.stride]; clipped = nf < end ? nf : end; }
                if (clipped <= start) continue;
                s_end = clipped; has = true; ev = this_ev; id = song.note_id[this_ev];
                break;
            }
        }
        if (has) {
            const uint32_t changed = tr.has_note ? (id != tr.note_id ? 1u : 0u) : 1u;  // :96-99
            emit(start, s_end, ev, changed);
            tr.has_note = 1; tr.note_id = id; tr.ev = ev;                             // defer self.note = note (:91)
        }
        start = s_end;
    }
}

// ---- live banks (k_voice_bank_schedule_live): the events of a buffer are pushed from outside (ImpulseQueue, notes.zig:72-128)
// One call's batch, sorted by instrument into CSR, is viewed through ZsSong (`t` unused): an impulse's `ev` is its index in the
// batch, and zs_dispatch_one / zs_trigger_buffer run on it unchanged.  The batch is gone by the next buffer, so a Trigger's carried
// note is not an index but the record itself: per-voice words, at most kZsMaxWords of them, and `ev` == kZsCarried names them.
// Between buffers every Trigger's `ev` is kZsCarried (zs_live_keep); a batch holds fewer than 2^32 - 1 impulses.
constexpr uint32_t kZsCarried = 0xffffffffu;
constexpr uint32_t kZsMaxWords = 16;        // ZH_MAX_PARAMS_SIZE / 4
struct ZsCarried {
    uint32_t *words;           // word w of ONE voice's carried record at index w * stride
    size_t stride;
};

// ImpulseQueue.push for the impulses [begin, end) of one instrument in push order, then consume, each accepted impulse handed
// straight to the dispatcher.  A push is dropped when 32 are accepted (:108-111) or when its frame is below the last accepted
// one's (:112-118); an accepted one takes event_id = next_event_id++ (:119-126).  Returns the number of list entries.
ZS_HD uint32_t zs_push_dispatch(const ZsSong &batch, const uint32_t *frame, uint32_t begin, uint32_t end, uint64_t &next_event_id,
                                const ZsSlots &sl, const ZsList &list) {
    uint32_t accepted = 0, listed = 0, last = 0;
    for (uint32_t ev = begin; ev < end && accepted < kZsMaxImpulses; ev++) {
        const uint32_t f = frame[ev];
        if (accepted > 0 && f < last) continue;
        last = f; accepted += 1;
        const uint64_t event_id = next_event_id;
        next_event_id += 1;
        listed = zs_dispatch_one(sl, list, listed, f, ev, batch.note_id[ev], zs_note_on(batch, ev), event_id);
    }
    return listed;
}

// word w of the record a sub-span's paint takes: the carried record's, or the batch's
ZS_HD uint32_t zs_live_word(const ZsSong &batch, const ZsCarried &c, uint32_t ev, uint32_t w) {
    return ev == kZsCarried ? c.words[w * c.stride] : batch.rec[(size_t)ev * batch.words + w];
}
ZS_HD bool zs_live_note_on(const ZsSong &batch, const ZsCarried &c, uint32_t ev) {
    return ((zs_live_word(batch, c, ev, batch.on_word) >> batch.on_shift) & 0xffu) != 0;
}
// after a voice's Trigger loop: the record of the note it ends on moves from the batch into the voice's carried words
ZS_HD void zs_live_keep(ZsTrigger &tr, const ZsSong &batch, const ZsCarried &c) {
    if (!tr.has_note || tr.ev == kZsCarried) return;
    for (uint32_t w = 0; w < batch.words; w++) c.words[w * c.stride] = batch.rec[(size_t)tr.ev * batch.words + w];
    tr.ev = kZsCarried;
}
