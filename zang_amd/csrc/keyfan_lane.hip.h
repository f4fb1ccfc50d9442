// keyfan_lane.hip.h -- the per-lane steps of the key fan-out stage (keyfan.hip), written once as __host__ __device__ functions so
// that the same text runs in a CPU harness (tests/cpp/keyfan_lane_host.cpp).  One call of keyfan_paint is ONE key's share of one
// call of Polyphony.paint (examples/example_polyphony.zig:61-92) without its instrument: the push at frame 0 when the key's bit
// differs from `down` (:70-77) and the key's own Trigger over the outer sub-span (:81-82; src/zang/trigger.zig:80-196), its
// sub-span handed to `emit`.  Nothing is stored per impulse: the key's queue holds at most the one impulse of this call, at frame
// 0, which no walk position is below -- so the Trigger's walk is one sub-span over the whole of [start, end): the pushed note if
// there is one (taken at the walk's position, where the reference asserts at trigger.zig:161), else the carried note, else none.
#pragma once
#include "span_stage.hip.h"
#define KEYFAN_HD STAGE_HD

constexpr uint32_t kKeyfanMaxKeys = 64;     // the held keys travel as two 32-bit record words

// words per voice, [word][voice]
enum { KS_NEXT_ID_LO = 0, KS_NEXT_ID_HI, KS_DOWN, KS_HAS_NOTE, KS_NOTE_ID_LO, KS_NOTE_ID_HI, KS_FREQ, KS_NOTE_ON, kKeyfanState };

struct KeyfanLane {
    uint64_t next_id;          // the Voice's IdGenerator (:37), 1 at init
    uint32_t down;             // :35
    uint32_t has_note;         // the Voice's Trigger's note (trigger.zig:41) ...
    uint64_t note_id;
    uint32_t freq_bits;        // ... and its params: freq as its bits, so that a lane moves no float
    uint32_t note_on;
};
KEYFAN_HD void keyfan_init(KeyfanLane &s) { s = KeyfanLane{1, 0, 0, 0, 0, 0}; }              // :50-56
KEYFAN_HD void keyfan_load(KeyfanLane &s, const uint32_t *w, size_t n, size_t v) {
    auto at = [&](int k) { return w[(size_t)k * n + v]; };
    s.next_id = at(KS_NEXT_ID_LO) | ((uint64_t)at(KS_NEXT_ID_HI) << 32);
    s.down = at(KS_DOWN);
    s.has_note = at(KS_HAS_NOTE);
    s.note_id = at(KS_NOTE_ID_LO) | ((uint64_t)at(KS_NOTE_ID_HI) << 32);
    s.freq_bits = at(KS_FREQ);
    s.note_on = at(KS_NOTE_ON);
}
KEYFAN_HD void keyfan_store(const KeyfanLane &s, uint32_t *w, size_t n, size_t v) {
    auto put = [&](int k, uint32_t x) { w[(size_t)k * n + v] = x; };
    put(KS_NEXT_ID_LO, (uint32_t)s.next_id); put(KS_NEXT_ID_HI, (uint32_t)(s.next_id >> 32));
    put(KS_DOWN, s.down);
    put(KS_HAS_NOTE, s.has_note);
    put(KS_NOTE_ID_LO, (uint32_t)s.note_id); put(KS_NOTE_ID_HI, (uint32_t)(s.note_id >> 32));
    put(KS_FREQ, s.freq_bits);
    put(KS_NOTE_ON, s.note_on);
}

// A stage's table (span_stage.hip.h StageRows) with note_on a second time as bytes, [row][voice] beside the table's rows: the
// plane zh_span_table has (zh_nice_paint_spans, zh_pmosc_paint_spans).  The Rows of a StageWriterT.
struct KeyfanRows {
    StageRows r;
    uint32_t *start, *end;                                            // r.start, r.end: what StageWriterT stores through
    uint8_t *note_on8;
    KEYFAN_HD void freq_on(size_t idx, uint32_t freq_bits, uint32_t note_on, uint32_t nic) const {
        r.freq_on(idx, freq_bits, note_on, nic);
        note_on8[idx] = (uint8_t)(note_on ? 1 : 0);
    }
};

// One key's share of one Polyphony.paint call over the outer sub-span [start, end): `bit` = params.note_held[key], freq_bits = the
// key's frequency.  emit(sub_start, sub_end, freq_bits, note_on, note_id_changed) for the sub-span the instrument is painted over.
template <class Emit>
KEYFAN_HD void keyfan_paint(KeyfanLane &s, uint32_t freq_bits, uint32_t bit, uint32_t start, uint32_t end, Emit &&emit) {
    if (bit != s.down) {                                              // :70-77: push(0, nextId(), {freq, note_on = bit})
        const uint64_t id = s.next_id++;
        s.down = bit;
        if (start >= end) return;                                     // trigger.zig:81: no walk; consume() (:81) emptied the queue
        const uint32_t changed = s.has_note ? (id != s.note_id ? 1u : 0u) : 1u;   // trigger.zig:96-99
        emit(start, end, freq_bits, bit, changed);
        s.has_note = 1; s.note_id = id; s.freq_bits = freq_bits; s.note_on = bit;
    } else if (s.has_note && start < end) {                           // carryOver, trigger.zig:107-137: no impulse, to the end
        emit(start, end, s.freq_bits, s.note_on, 0u);
    }
}

// One voice's buffer: key `key`'s share of Polyphony.paint per outer sub-span that holds a note (MainModule.paint :137-145).  The
// outer table's column: count, and start / end / the two mask words at index k * stride.  A sub-span the outer Trigger cannot have
// made (end < start, end > out_len) ends the list.
template <class Emit>
KEYFAN_HD void keyfan_buffer(KeyfanLane &s, uint32_t freq_bits, uint32_t key, uint32_t out_len, uint32_t count, const uint32_t *start,
                             const uint32_t *end, const uint32_t *held_lo, const uint32_t *held_hi, size_t stride, Emit &&emit) {
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t s0 = start[k * stride], s1 = end[k * stride];
        if (s1 < s0 || s1 > out_len) break;
        const uint64_t held = held_lo[k * stride] | ((uint64_t)held_hi[k * stride] << 32);
        keyfan_paint(s, freq_bits, (uint32_t)((held >> key) & 1u), s0, s1, emit);
    }
}
