"""The yardstick of the key-per-voice polyphony tests; holds no tests.  examples/example_polyphony.zig restated line by line in
Python, from the Zig alone: MainModule's ImpulseQueue and Trigger over the held-key records (:129-145, :166-178), the space bar's
dec_mode (:167-169), and Polyphony.paint (:61-92) with every key's OWN ImpulseQueue, IdGenerator and Trigger -- a real push(0, ...)
when the key's flag differs from `down`, a real consume(), and the Trigger's walk over the outer sub-span; nothing of it is worked
out in closed form.  ImpulseQueue, Trigger and the stage's table are tests/span_reference.py's: where the reference is undefined,
an impulse below the Trigger's position (its assert, trigger.zig:161 -- frame 0 in any outer sub-span that does not start at 0) is
taken at the position.  render() paints each voice's sub-spans with the oracle's zo_nice_paint onto the player's one bus and takes
it through zo_decimator_paint, or zo_add_into for mode 0 (:147-163).  A record is the held-key MASK (bit i = note_held[i]); bits at
or above the key count stand for no key."""
import ctypes as C

import numpy as np

from tests.span_reference import ImpulseQueue, Trigger, bits, same_table, table  # noqa: F401  (for the tests)

f32 = np.float32
SAMPLE_RATE = 48000.0                                                          # :11
DEC_RATES = (None, 6000.0, 5000.0, 4000.0, 3000.0, 2000.0, 1000.0)             # :151-158; mode 0: addInto (:161-163)


class Voice:
    """:34-40 without the instrument"""

    def __init__(self):
        self.down, self.iq, self.next_id, self.trigger = False, ImpulseQueue(), 1, Trigger()   # :50-56 (IdGenerator.init: 1)

    def words(self):
        """the stage's state, in zh_keyfan_state's order; freq as its bits"""
        note = self.trigger.note
        return [self.next_id, int(self.down), int(note is not None), note[0] if note else 0, bits(note[1][0]) if note else 0,
                int(note[1][1]) if note else 0]


class Polyphony:
    """:26-93 without the instruments: paint -> per key, the sub-spans its instrument is painted over"""

    def __init__(self, key_freqs):
        self.key_freqs = [f32(x) for x in key_freqs]
        self.voices = [Voice() for _ in self.key_freqs]                        # :48-57

    def paint(self, start, end, mask):
        """-> [key] -> [(s, e, (freq, note_on), note_id_changed)]"""
        for i, v in enumerate(self.voices):                                    # :68-78
            held = bool((mask >> i) & 1)
            if held != v.down:
                nid = v.next_id
                v.next_id += 1
                v.iq.push(0, nid, (self.key_freqs[i], held))
                v.down = held
        return [v.trigger.spans(start, end, v.iq.consume()) for v in self.voices]   # :80-91


class MainModule:
    """:99-179 for one player: keyEvent, the space bar, and paint down to every key's list of sub-spans"""

    def __init__(self, key_freqs):
        self.n_keys = len(key_freqs)
        self.mask = 0                                                          # current_params.note_held, :118
        self.iq, self.next_id, self.trigger = ImpulseQueue(), 1, Trigger()
        self.polyphony = Polyphony(key_freqs)
        self.dec_mode = 0

    def key_event(self, key_index, down, frame, stray=0):                      # :171-176
        """`stray`: bits set in the pushed mask beside the keys' (what a caller's record can hold, not what keyEvent makes)"""
        self.mask = (self.mask | (1 << key_index)) if down else (self.mask & ~(1 << key_index))
        note_id = self.next_id
        self.next_id += 1
        self.iq.push(frame, note_id, self.mask | stray)
        return note_id, self.mask | stray

    def space(self):                                                           # :167-169
        self.dec_mode = (self.dec_mode + 1) % 7
        return self.dec_mode

    def schedule(self, out_len):
        """:137-145 -> (outer sub-spans, [key] -> inner sub-spans in paint order)"""
        outer = self.trigger.spans(0, out_len, self.iq.consume())
        inner = [[] for _ in range(self.n_keys)]
        for s, e, mask, _ in outer:
            for k, spans in enumerate(self.polyphony.paint(s, e, mask)):
                inner[k] += spans
        return outer, inner


class Bus:
    """one player's instruments (:38, Instrument.init(0.3) :54) and Decimator (:124) in the oracle"""

    def __init__(self, o, n_keys, color=0.3):
        L = o.lib()
        self.nice = [o.NiceInstrument() for _ in range(n_keys)]
        for st in self.nice:
            L.zo_nice_init(C.byref(st), float(color))
        self.dec = o.Decimator()
        L.zo_decimator_init(C.byref(self.dec))


def render(o, buses, players_inner, dec_modes, frames):
    """MainModule.paint into a zeroed output for every player: players_inner[p][key] = the key's sub-spans -> audio [N][frames]"""
    L = o.lib()
    audio = np.zeros((len(buses), frames), f32)
    t0, t1 = np.zeros(frames, f32), np.zeros(frames, f32)
    for p, bus in enumerate(buses):
        mix = np.zeros(frames, f32)                                            # zang.zero(span, temps[2]), :135
        for key, spans in enumerate(players_inner[p]):                         # :80-91, onto the one temps[2]
            for s, e, (freq, on), changed in spans:
                L.zo_nice_paint(C.byref(bus.nice[key]), s, e, o.fptr(mix), o.fptr(t0), o.fptr(t1), int(bool(changed)), SAMPLE_RATE,
                                float(f32(freq)), int(bool(on)))
        if dec_modes[p] > 0:                                                   # :147-160
            L.zo_decimator_paint(C.byref(bus.dec), 0, frames, o.fptr(audio[p]), SAMPLE_RATE, o.fptr(mix), DEC_RATES[dec_modes[p]])
        else:
            L.zo_add_into(0, frames, o.fptr(audio[p]), o.fptr(mix))            # :162
    return audio
