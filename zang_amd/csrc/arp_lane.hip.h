// arp_lane.hip.h -- the per-lane steps of the arpeggiator stage (arp.hip), written once as __host__ __device__ functions so that
// the same text runs in a CPU harness (tests/cpp/arp_lane_host.cpp).  One call of arp_paint is one call of Arpeggiator.paint
// (examples/example_arpeggiator.zig:49-117) without its instrument: the tick loop (:68-102), the clock's step back (:104) and the
// inner Trigger's walk (:106-107; src/zang/trigger.zig:80-196) over the outer sub-span, each sub-span handed to `emit`.
// Nothing is stored per impulse.  Within one call the held keys do not change, so either every tick pushes or none does; the
// pushed frames are next_frame + i * note_duration and the ids next_id + i, and the key of impulse i + 1 follows from impulse i's
// (arp_next_key).  The walk steps through them in order; state after the ticks (last_note, next_id, the ones past the queue's 32
// included) is computed up front.
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ARP_HD __host__ __device__ inline
#else
#define ARP_HD inline
#endif

constexpr uint32_t kArpMaxImpulses = 32;    // the inner ImpulseQueue's cap (notes.zig:73-74)
constexpr uint32_t kArpMaxKeys = 64;        // the held keys travel as two 32-bit record words

// words per player, [word][player]
enum { AS_NEXT_FRAME_LO = 0, AS_NEXT_FRAME_HI, AS_NEXT_ID_LO, AS_NEXT_ID_HI, AS_LAST_NOTE, AS_HAS_NOTE, AS_NOTE_ID_LO, AS_NOTE_ID_HI,
       AS_FREQ, AS_NOTE_ON, kArpState };

struct ArpLane {
    uint64_t next_frame;       // :35
    uint64_t next_id;          // the IdGenerator (:32), 1 at init
    int32_t last_note;         // :36, -1 = null
    uint32_t has_note;         // the inner Trigger's note (trigger.zig:41) ...
    uint64_t note_id;
    uint32_t freq_bits;        // ... and its params: freq as its bits, so that a lane moves no float
    uint32_t note_on;
};
ARP_HD void arp_init(ArpLane &s) { s = ArpLane{0, 1, -1, 0, 0, 0, 0}; }                     // :38-47
ARP_HD void arp_load(ArpLane &s, const uint32_t *w, size_t n, size_t v) {
    auto at = [&](int k) { return w[(size_t)k * n + v]; };
    s.next_frame = at(AS_NEXT_FRAME_LO) | ((uint64_t)at(AS_NEXT_FRAME_HI) << 32);
    s.next_id = at(AS_NEXT_ID_LO) | ((uint64_t)at(AS_NEXT_ID_HI) << 32);
    s.last_note = (int32_t)at(AS_LAST_NOTE);
    s.has_note = at(AS_HAS_NOTE);
    s.note_id = at(AS_NOTE_ID_LO) | ((uint64_t)at(AS_NOTE_ID_HI) << 32);
    s.freq_bits = at(AS_FREQ);
    s.note_on = at(AS_NOTE_ON);
}
ARP_HD void arp_store(const ArpLane &s, uint32_t *w, size_t n, size_t v) {
    auto put = [&](int k, uint32_t x) { w[(size_t)k * n + v] = x; };
    put(AS_NEXT_FRAME_LO, (uint32_t)s.next_frame); put(AS_NEXT_FRAME_HI, (uint32_t)(s.next_frame >> 32));
    put(AS_NEXT_ID_LO, (uint32_t)s.next_id); put(AS_NEXT_ID_HI, (uint32_t)(s.next_id >> 32));
    put(AS_LAST_NOTE, (uint32_t)s.last_note);
    put(AS_HAS_NOTE, s.has_note);
    put(AS_NOTE_ID_LO, (uint32_t)s.note_id); put(AS_NOTE_ID_HI, (uint32_t)(s.note_id >> 32));
    put(AS_FREQ, s.freq_bits);
    put(AS_NOTE_ON, s.note_on);
}

// :56  `@intFromFloat(0.03 * params.sample_rate)`: the comptime 0.03 becomes an f32, the product is rounded once.  false where the
// reference loops for ever (0) or its conversion is undefined (NaN, negative, 2^31 and above).
ARP_HD bool arp_note_duration(float sample_rate, uint32_t &nd) {
    const float p = 0.03f * sample_rate;
    if (!(p >= 1.0f && p < 2147483648.0f)) return false;
    nd = (uint32_t)p;
    return true;
}

// :69-82 with a non-empty mask (bits at or above n_keys clear): the first held key at (last + 1 + i) % n_keys, i = 0, 1, ...
ARP_HD int32_t arp_next_key(int32_t last, uint64_t mask, uint32_t n_keys) {
    uint32_t start = (uint32_t)(last + 1);                            // null: 0
    if (start >= n_keys) start = 0;                                   // (n_keys - 1 + 1) % n_keys
    const uint64_t from = mask & (~0ull << start);
    return (int32_t)__builtin_ctzll(from ? from : mask);
}
// last_note after t >= 1 ticks that each found a key: the first tick lands on a held key, every further one moves to the next held
// key in a cycle of popcount(mask)
ARP_HD int32_t arp_advance_key(int32_t last, uint64_t mask, uint32_t n_keys, uint64_t t) {
    int32_t k = arp_next_key(last, mask, n_keys);
    uint32_t more = (uint32_t)((t - 1) % (uint64_t)__builtin_popcountll(mask));
    while (more--) k = arp_next_key(k, mask, n_keys);
    return k;
}

// One Arpeggiator.paint call: outer sub-span [start, end) of a buffer of out_len frames, `held` = params.note_held as a mask,
// nd = note_duration.  emit(sub_start, sub_end, freq_bits, note_on, note_id_changed) per inner sub-span, in order.
template <class Emit>
ARP_HD void arp_paint(ArpLane &s, const uint32_t *key_freq_bits, uint32_t n_keys, uint64_t held, uint32_t nd, uint32_t out_len, uint32_t start,
                      uint32_t end, Emit &&emit) {
    const uint64_t mask = n_keys >= 64 ? held : held & ((1ull << n_keys) - 1);
    const bool on = mask != 0;
    // ---- :68-104
    const uint64_t f0 = s.next_frame, id0 = s.next_id;
    const int32_t last0 = s.last_note;
    const uint64_t ticks = f0 < out_len ? (out_len - f0 + nd - 1) / nd : 0;
    s.next_frame = f0 + ticks * nd - out_len;
    const bool pushes = ticks > 0 && (on || last0 >= 0);              // :84, :92; neither: nothing pushed, no id drawn
    uint32_t n_imp = 0;
    if (pushes) {
        n_imp = ticks < kArpMaxImpulses ? (uint32_t)ticks : kArpMaxImpulses;
        s.next_id = id0 + ticks;                                      // nextId() is evaluated for a push the queue drops too
        if (on) s.last_note = arp_advance_key(last0, mask, n_keys, ticks);   // :91
    }
    // impulse i < n_imp: frame f0 + i * nd (< out_len), id id0 + i, note_on = on, key = cur_key once cur == i
    uint32_t cur = 0;
    int32_t cur_key = !pushes ? 0 : on ? arp_next_key(last0, mask, n_keys) : last0;
    auto frame_of = [&](uint32_t i) { return (uint32_t)(f0 + (uint64_t)i * nd); };
    // ---- :106-107: Trigger.counter(span, iq.consume()) and the Trigger.next loop
    uint32_t pos = start;
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
                if (f >= end) break;                                  // :144-150: the walk ends, the impulse is lost
                if (f > pos) { s_end = f; break; }                    // :152-159 the gap before it
                // f <= pos.  f < pos trips the reference's assert (:161): taken at the walk's position, as zs_trigger_buffer does
                const uint64_t this_id = id0 + cur;
                const int32_t this_key = cur_key;
                cur++;                                                // :163
                if (on && cur < n_imp) cur_key = arp_next_key(cur_key, mask, n_keys);
                uint32_t clipped = end;                               // :167-171
                if (cur < n_imp) { const uint32_t nf = frame_of(cur); clipped = nf < end ? nf : end; }
                if (clipped <= pos) continue;                         // :173-178
                s_end = clipped; has = true; id = this_id; fb = key_freq_bits[this_key]; non = on ? 1u : 0u;
                break;
            }
        }
        if (has) {
            const uint32_t changed = s.has_note ? (id != s.note_id ? 1u : 0u) : 1u;   // :96-99
            emit(pos, s_end, fb, non, changed);
            s.has_note = 1; s.note_id = id; s.freq_bits = fb; s.note_on = non;      // defer self.note = note (:91)
        }
        pos = s_end;
    }
}

// One player's buffer: Arpeggiator.paint per outer sub-span that holds a note (MainModule.paint :153-156).  The outer table's
// column: count, and start / end / the two mask words at index k * stride.  A sub-span the outer Trigger cannot have made (end <
// start, end > out_len) ends the list.
template <class Emit>
ARP_HD void arp_buffer(ArpLane &s, const uint32_t *key_freq_bits, uint32_t n_keys, uint32_t nd, uint32_t out_len, uint32_t count,
                       const uint32_t *start, const uint32_t *end, const uint32_t *held_lo, const uint32_t *held_hi, size_t stride, Emit &&emit) {
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t s0 = start[k * stride], s1 = end[k * stride];
        if (s1 < s0 || s1 > out_len) break;
        const uint64_t held = held_lo[k * stride] | ((uint64_t)held_hi[k * stride] << 32);
        arp_paint(s, key_freq_bits, n_keys, held, nd, out_len, s0, s1, emit);
    }
}
