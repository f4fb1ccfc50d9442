// subsong_lane.hip.h -- the per-lane steps of the subsong stage (subsong.hip), written once as __host__ __device__ functions so
// that the same text runs in a CPU harness (tests/cpp/subsong_lane_host.cpp).  One call of subsong_paint is one call of
// SubtrackPlayer.paint (examples/example_subsong.zig:122-144) without its instrument: the reset (:130-133), NoteTracker.consume
// (src/zang/notes.zig:162-206) over the sub-span and the inner Trigger's walk (:135-136; src/zang/trigger.zig:80-196), each inner
// sub-span handed to `emit` with the frequency of :140.
// Nothing is stored per impulse.  The song is chronological, so the events one call consumes are next_song_event .. the first
// whose t is not below end_t; impulse i of the call is event first + i, and its frame is a function of that event's t and of the
// clock before the call (subsong frame_of), evaluated where the walk asks for it.  f32 throughout, no contraction.
#pragma once
#include "span_stage.hip.h"
#define SS_HD STAGE_HD

constexpr uint32_t kSubsongMaxImpulses = 32;     // NoteTracker's arrays (notes.zig:142-143)
constexpr uint32_t kSubsongNoMelody = 0xffffffffu;   // the latched melody of a player that plays none (an index at or above K)

// words per player, [word][player]
enum { SS_NEXT = 0, SS_T, SS_MELODY, SS_HAS_NOTE, SS_NOTE_ID_LO, SS_NOTE_ID_HI, SS_FREQ, SS_NOTE_ON, kSubsongState };

struct SubsongLane {
    uint32_t next;             // NoteTracker.next_song_event (notes.zig:140)
    uint32_t t_bits;           // NoteTracker.t (:141) as its bits
    uint32_t melody;           // which of the kit's melodies `song` (:139) is; kSubsongNoMelody = an empty one
    uint32_t has_note;         // the inner Trigger's note (trigger.zig:41) ...
    uint64_t note_id;
    uint32_t freq_bits;        // ... and its params: the song's RAW freq as its bits (scaled at every emit, :140)
    uint32_t note_on;
};
// a kit as the lane reads it: melody m = events [offsets[m], offsets[m + 1])
struct SubsongKitP {
    uint32_t K;
    const uint32_t *offsets;                                          // [K + 1]
    const uint32_t *t_bits, *id_lo, *id_hi, *freq_bits, *note_on;     // [events]
};

SS_HD float ss_float(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
SS_HD uint32_t ss_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
// @intFromFloat, defined where the reference's is not as zf32_to_u32 (zmath.hip.h) defines it: NaN and below 0 -> 0, saturating
SS_HD uint32_t ss_f32_to_u32(float v) {
    if (!(v == v)) return 0u;
    if (v <= 0.0f) return 0u;
    if (v >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)v;
}

// SubtrackPlayer.init (:104-120): the tracker at the song's start, the trigger without a note.  The reference has one song: the
// kit's melody 0 (none where the kit is empty).
SS_HD void subsong_init(SubsongLane &s, uint32_t K) { s = SubsongLane{0, 0, K ? 0u : kSubsongNoMelody, 0, 0, 0, 0}; }
SS_HD void subsong_load(SubsongLane &s, const uint32_t *w, size_t n, size_t v) {
    auto at = [&](int k) { return w[(size_t)k * n + v]; };
    s.next = at(SS_NEXT);
    s.t_bits = at(SS_T);
    s.melody = at(SS_MELODY);
    s.has_note = at(SS_HAS_NOTE);
    s.note_id = at(SS_NOTE_ID_LO) | ((uint64_t)at(SS_NOTE_ID_HI) << 32);
    s.freq_bits = at(SS_FREQ);
    s.note_on = at(SS_NOTE_ON);
}
SS_HD void subsong_store(const SubsongLane &s, uint32_t *w, size_t n, size_t v) {
    auto put = [&](int k, uint32_t x) { w[(size_t)k * n + v] = x; };
    put(SS_NEXT, s.next);
    put(SS_T, s.t_bits);
    put(SS_MELODY, s.melody);
    put(SS_HAS_NOTE, s.has_note);
    put(SS_NOTE_ID_LO, (uint32_t)s.note_id); put(SS_NOTE_ID_HI, (uint32_t)(s.note_id >> 32));
    put(SS_FREQ, s.freq_bits);
    put(SS_NOTE_ON, s.note_on);
}

// The stage's table as five arrays of their own, [row][player] (the CPU harness's), under the writer the kernel emits through
struct SubsongRowsP {
    uint32_t *start, *end, *freq, *note_on;
    uint8_t *changed;
    SS_HD void freq_on(size_t idx, uint32_t freq_bits, uint32_t on, uint32_t nic) const {
        freq[idx] = freq_bits; note_on[idx] = on; changed[idx] = (uint8_t)nic;
    }
};
using SubsongEmit = StageWriterT<SubsongRowsP>;

// One SubtrackPlayer.paint call: outer sub-span [start, end), start < end, with the outer note's freq, note_on, note_id_changed
// and melody.  emit(sub_start, sub_end, freq_bits, note_on, note_id_changed) per inner sub-span, in order.
template <class Emit>
SS_HD void subsong_paint(SubsongLane &s, const SubsongKitP &kit, float base_freq, float sample_rate, uint32_t start, uint32_t end,
                         float freq_o, bool on_o, bool nic_o, uint32_t melody_o, Emit &&emit) {
    const bool outer_new = on_o && nic_o;
    if (outer_new) {                                                  // :130-133 tracker.reset(), trigger.reset()
        s.next = 0; s.t_bits = 0;
        s.has_note = 0; s.note_id = 0; s.freq_bits = 0; s.note_on = 0;
        s.melody = melody_o < kit.K ? melody_o : kSubsongNoMelody;
    }
    uint32_t lo = 0, n_ev = 0;
    if (s.melody < kit.K) { lo = kit.offsets[s.melody]; n_ev = kit.offsets[s.melody + 1] - lo; }
    // ---- :134 NoteTracker.consume (notes.zig:162-206)
    const uint32_t out_len = end - start;                             // :169 the SUB-SPAN's length
    const float t0 = ss_float(s.t_bits);
    const float buf_time = (float)out_len / sample_rate;              // :170
    const float end_t = t0 + buf_time;                                // :172
    const uint32_t first = s.next;
    uint32_t nx = first;
    while (nx < n_ev && ss_float(kit.t_bits[lo + nx]) < end_t) nx++;  // :174-198
    s.next = nx;                                                      // a 33rd event advances it and is dropped
    s.t_bits = ss_bits(end_t);                                        // :200
    const uint32_t taken = nx - first;
    const uint32_t n_imp = taken < kSubsongMaxImpulses ? taken : kSubsongMaxImpulses;
    auto frame_of = [&](uint32_t i) {                                 // :179-188 for impulse i < n_imp
        const float note_t = ss_float(kit.t_bits[lo + first + i]);
        const float f = (note_t - t0) / buf_time;
        const uint32_t rel = ss_f32_to_u32(f * (float)out_len);
        return start + (rel < out_len - 1 ? rel : out_len - 1);
    };
    // ---- :135-136 Trigger.counter(span, iap) and the Trigger.next loop
    uint32_t cur = 0, pos = start;
    while (pos < end) {
        bool has = false, found = false;
        uint32_t s_end = end, fb = 0, non = 0;
        uint64_t id = 0;
        if (s.has_note) {                                             // carryOver, trigger.zig:107-137
            if (cur < n_imp) {
                const uint32_t nf = frame_of(cur);
                if (nf > pos) { s_end = nf < end ? nf : end; found = true; }
            } else found = true;
            if (found) { has = true; id = s.note_id; fb = s.freq_bits; non = s.note_on; }
        }
        if (!found) {                                                 // getNextNoteSpan :139-196
            while (cur < n_imp) {
                const uint32_t f = frame_of(cur);
                if (f >= end) break;                                  // :144-150 (consume's @min keeps every frame below end)
                if (f > pos) { s_end = f; break; }                    // :152-159 the gap before it
                // f <= pos.  f < pos (a clock running backwards: a negative sample rate) trips the reference's assert (:161):
                // taken at the walk's position, as zh_trigger_next defines it
                const uint32_t e = lo + first + cur;
                cur++;                                                // :163
                uint32_t clipped = end;                               // :167-171
                if (cur < n_imp) { const uint32_t nf = frame_of(cur); clipped = nf < end ? nf : end; }
                if (clipped <= pos) continue;                         // :173-178
                s_end = clipped; has = true;
                id = kit.id_lo[e] | ((uint64_t)kit.id_hi[e] << 32); fb = kit.freq_bits[e]; non = kit.note_on[e] ? 1u : 0u;
                break;
            }
        }
        if (has) {
            const bool inner_changed = s.has_note ? id != s.note_id : true;    // trigger.zig:96-99: the song's note_id
            const float prod = ss_float(fb) * freq_o;                          // :140, two roundings in this order
            const float freq = prod / base_freq;
            emit(pos, s_end, ss_bits(freq), non, (outer_new || inner_changed) ? 1u : 0u);   // :137
            s.has_note = 1; s.note_id = id; s.freq_bits = fb; s.note_on = non; // defer self.note = note (:91), the RAW freq
        }
        pos = s_end;
    }
}

// One player's buffer: SubtrackPlayer.paint per outer sub-span (MainModule.paint :176-185).  The outer table's column: count, and
// start / end / note_id_changed / freq / note_on / melody at index k * stride.  A sub-span the outer Trigger cannot have made
// (end <= start, end > out_len) ends the list.
template <class Emit>
SS_HD void subsong_buffer(SubsongLane &s, const SubsongKitP &kit, float base_freq, float sample_rate, uint32_t out_len, uint32_t count,
                          const uint32_t *start, const uint32_t *end, const uint8_t *nic, const float *freq, const uint32_t *note_on,
                          const uint32_t *melody, size_t stride, Emit &&emit) {
    for (uint32_t k = 0; k < count; k++) {
        const size_t i = k * stride;
        const uint32_t s0 = start[i], s1 = end[i];
        if (s1 <= s0 || s1 > out_len) break;
        subsong_paint(s, kit, base_freq, sample_rate, s0, s1, freq[i], note_on[i] != 0, nic[i] != 0, melody[i], emit);
    }
}
