"""The yardstick of the arpeggiator tests; holds no tests.  examples/example_arpeggiator.zig restated line by line in Python, from
the Zig alone: MainModule's ImpulseQueue and Trigger over the held-key records (:147-167), Arpeggiator.paint's tick loop with its
own ImpulseQueue and IdGenerator (:56-104) and the inner Trigger (:106-107), each sub-span painted by the oracle's
zo_hard_square_paint plus zo_add_scalar_into (:108-115).  ImpulseQueue, Trigger and the stage's table are tests/span_reference.py's:
impulses are stored in lists, as the reference stores them, and where the reference is undefined, an impulse below the Trigger's
position (its assert, trigger.zig:161) is taken at the position."""
import ctypes as C

import numpy as np

from tests.span_reference import MAX_IMPULSES, ImpulseQueue, Trigger, same_table, table  # noqa: F401  (for the tests)

f32 = np.float32


def note_duration(sample_rate):
    """:56 -- the comptime 0.03 as an f32 times the f32 sample rate, rounded once, truncated; None where the reference loops for
    ever or its @intFromFloat is undefined"""
    with np.errstate(all="ignore"):
        p = f32(0.03) * f32(sample_rate)
    if not (p >= 1.0 and p < 2147483648.0):
        return None
    return int(p)


def note_duration_f64(sample_rate):
    """what a careless restatement computes: the same f32 constant, the product in f64"""
    return int(float(f32(0.03)) * float(f32(sample_rate)))


class Arpeggiator:
    """:23-118 without the instrument: paint -> the sub-spans the instrument is painted over"""

    def __init__(self, key_freqs):
        self.key_freqs = [f32(x) for x in key_freqs]
        self.iq, self.next_id, self.trigger = ImpulseQueue(), 1, Trigger()     # :40-43 (IdGenerator.init: 1)
        self.next_frame, self.last_note = 0, None                              # :44-45
        # what the tests ask the model about its own run: generated frames below the outer sub-span's start / at or above its end
        self.stats = {"below_start": 0, "at_or_above_end": 0, "dropped_pushes": 0, "calls": 0}

    def _next_id(self):
        i = self.next_id
        self.next_id += 1
        return i

    def paint(self, start, end, out_len, sample_rate, note_held):
        """note_held: a list of n_keys bools -> [(s, e, (freq, note_on), note_id_changed)]"""
        nd = note_duration(sample_rate)
        n = len(self.key_freqs)
        self.stats["calls"] += 1
        while self.next_frame < out_len:                                       # :68
            start_i = self.last_note + 1 if self.last_note is not None else 0  # :70-73
            nxt = None
            for i in range(n):                                                 # :74-80
                index = (start_i + i) % n
                if note_held[index]:
                    nxt = index
                    break
            if nxt is not None:                                                # :84-91
                self._push(self.next_frame, self._next_id(), (self.key_freqs[nxt], True))
                self.last_note = nxt
            elif self.last_note is not None:                                   # :92-99
                self._push(self.next_frame, self._next_id(), (self.key_freqs[self.last_note], False))
            self.next_frame += nd                                              # :101
        self.next_frame -= out_len                                             # :104
        impulses = self.iq.consume()
        self.stats["below_start"] += sum(f < start for f, _, _ in impulses)
        self.stats["at_or_above_end"] += sum(f >= end for f, _, _ in impulses)
        return self.trigger.spans(start, end, impulses)                        # :106-107

    def _push(self, frame, note_id, params):
        before = len(self.iq.items)
        self.iq.push(frame, note_id, params)
        self.stats["dropped_pushes"] += len(self.iq.items) == before

    def words(self):
        """the stage's state, in zh_arp_state's order; freq as its bits"""
        note = self.trigger.note
        return [self.next_frame, self.next_id, -1 if self.last_note is None else self.last_note, int(note is not None),
                note[0] if note else 0, int(np.array([note[1][0] if note else 0.0], f32).view(np.uint32)[0]), int(note[1][1]) if note else 0]


class Player:
    """MainModule (:120-168) for one player: keyEvent, and paint down to the list of inner sub-spans"""

    def __init__(self, key_freqs):
        self.n_keys = len(key_freqs)
        self.note_held = [False] * self.n_keys                                 # :138
        self.iq, self.next_id, self.trigger = ImpulseQueue(), 1, Trigger()
        self.arp = Arpeggiator(key_freqs)

    def key_event(self, key_index, down, frame):                               # :159-167
        self.note_held[key_index] = bool(down)
        note_id = self.next_id
        self.next_id += 1
        self.iq.push(frame, note_id, list(self.note_held))
        return note_id, sum(1 << i for i, h in enumerate(self.note_held) if h)

    def schedule(self, out_len, sample_rate):
        """:153-156 -> (outer sub-spans, inner sub-spans in paint order)"""
        outer = self.trigger.spans(0, out_len, self.iq.consume())
        inner = []
        for s, e, held, _ in outer:
            inner += self.arp.paint(s, e, out_len, sample_rate, held)
        return outer, inner


class HardSquareVoice:
    """HardSquareInstrument's state (examples/modules.zig:259-260)"""

    def __init__(self, o):
        self.st = o.HardSquare()
        o.lib().zo_hard_square_init(C.byref(self.st))

    @property
    def cnt(self):
        return int(self.st.osc.cnt)


def hard_square_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, note_on, patch=None):
    """Instrument.paint (examples/modules.zig:269-288) and the addScalarInto of example_arpeggiator.zig:115; outputs = (out0, out1
    or None), temps = two rows or more; the signature of tests/lead_reference.py's paints"""
    L = o.lib()
    L.zo_hard_square_paint(C.byref(voice.st), start, end, o.fptr(outputs[0]), o.fptr(temps[0]), o.fptr(temps[1]), int(bool(nic)),
                           float(sample_rate), float(f32(freq)), int(bool(note_on)))
    if outputs[1] is not None:
        L.zo_add_scalar_into(start, end, o.fptr(outputs[1]), float(f32(freq)))


def render(o, voices, players_spans, frames, sample_rate):
    """MainModule.paint into zeroed outputs for every player: -> (audio, sync) [N][frames]"""
    N = len(players_spans)
    audio, sync = np.zeros((N, frames), f32), np.zeros((N, frames), f32)
    temps = [np.zeros(frames, f32) for _ in range(2)]
    for p, spans in enumerate(players_spans):
        for s, e, (freq, on), changed in spans:
            hard_square_paint(o, voices[p], s, e, (audio[p], sync[p]), temps, changed, sample_rate, freq, on)
    return audio, sync
