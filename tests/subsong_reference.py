"""The yardstick of the subsong tests; holds no tests.  examples/example_subsong.zig restated line by line in numpy f32, from the
Zig alone, with the two src/zang files it leans on: NoteTracker (src/zang/notes.zig:138-207), Trigger (src/zang/trigger.zig:26-198;
tests/span_reference.py's, with its ImpulseQueue and the stage's table),
SubtrackPlayer.paint (:122-144), MainModule's ImpulseQueue, Trigger and keyEvent (:170-201), and InnerInstrument.paint (:43-67) over
the oracle's modules.  Impulses are stored in lists here, as the reference stores them in its arrays of 32.
Where the reference is undefined: @intFromFloat of a NaN is 0 and saturates; an impulse below the Trigger's position (its assert,
trigger.zig:161; reached only by a clock that runs backwards) is taken at the position; a melody index outside the kit plays an
empty song."""
import ctypes as C

import numpy as np

from tests.span_reference import MAX_IMPULSES, ImpulseQueue, Trigger, bits, same_table, table  # noqa: F401  (for the tests)

f32 = np.float32
NO_MELODY = 0xffffffff


def int_from_float(x):
    """@intFromFloat to usize where it is defined; NaN and below zero -> 0, 2^32 and above -> 2^32 - 1"""
    if not (x == x) or x <= 0:
        return 0
    if x >= 4294967296.0:
        return 0xffffffff
    return int(x)


class NoteTracker:
    """notes.zig:138-207 over song = [(t, note_id, freq, note_on)]"""

    def __init__(self, song):
        self.song, self.next_song_event, self.t = song, 0, f32(0.0)            # :145-153
        self.stats = {"clamped": 0, "at_last": 0, "dropped": 0, "same_frame": 0}

    def reset(self):                                                           # :155-158
        self.next_song_event, self.t = 0, f32(0.0)

    def consume(self, sample_rate, start, end):
        impulses = []                                                          # :167 count = 0
        out_len = end - start                                                  # :169
        with np.errstate(all="ignore"):
            buf_time = f32(out_len) / f32(sample_rate)                         # :170
            end_t = self.t + buf_time                                          # :172
            for t, note_id, freq, note_on in self.song[self.next_song_event:]:   # :174
                note_t, params = f32(t), (f32(freq), bool(note_on))
                if not note_t < end_t:                                         # :178, :195-197
                    break
                f = (note_t - self.t) / buf_time                               # :179
                rel = int_from_float(f * f32(out_len))                         # :181
                self.stats["clamped"] += rel > out_len - 1                    # the @min below changes it
                self.stats["at_last"] += rel == out_len - 1
                rel = min(rel, out_len - 1)                                    # :180-183
                self.next_song_event += 1                                      # :186
                if len(impulses) < MAX_IMPULSES:                               # the arrays hold 32; further ones are dropped
                    self.stats["same_frame"] += bool(impulses) and impulses[-1][0] == start + rel
                    impulses.append((start + rel, note_id, params))            # :187-193
                else:
                    self.stats["dropped"] += 1
            self.t = f32(end_t)                                                # :200
        return impulses


class SubtrackPlayer:
    """:89-145 without the instrument, over a kit of songs: paint -> the sub-spans the instrument is painted over"""

    def __init__(self, kit, base_freq):
        self.kit, self.base_freq = kit, f32(base_freq)
        self.melody = 0 if kit else NO_MELODY                                  # the reference's one song
        self.tracker = NoteTracker(kit[0] if kit else [])                      # :109
        self.trigger = Trigger()                                               # :118
        self.stats = {"clamped": 0, "at_last": 0, "dropped": 0, "same_frame": 0, "resets": 0}

    def paint(self, start, end, note_id_changed, sample_rate, freq, note_on, melody):
        """-> [(s, e, (freq, note_on), new_note)]"""
        outer_new = bool(note_on) and bool(note_id_changed)
        if outer_new:                                                          # :130-133
            self.melody = melody if melody < len(self.kit) else NO_MELODY
            self._fold_stats()
            self.tracker = NoteTracker(self.kit[self.melody] if self.melody != NO_MELODY else [])   # reset() on the latched song
            self.trigger.reset()
            self.stats["resets"] += 1
        iap = self.tracker.consume(sample_rate, start, end)                    # :134
        rows = []
        for s, e, (f_i, on_i), changed in self.trigger.spans(start, end, iap):  # :135-136
            new_note = outer_new or changed                                    # :137
            with np.errstate(all="ignore"):
                scaled = (f32(f_i) * f32(freq)) / self.base_freq               # :140
            rows.append((s, e, (f32(scaled), bool(on_i)), new_note))
        return rows

    def _fold_stats(self):
        for k, v in self.tracker.stats.items():
            self.stats[k] += v
        self.tracker.stats = dict.fromkeys(self.tracker.stats, 0)

    def words(self):
        """the stage's state, in zh_subsong_state's order; t and freq as their bits"""
        note = self.trigger.note
        return [self.tracker.next_song_event, bits(self.tracker.t), self.melody, int(note is not None), note[0] if note else 0,
                bits(note[1][0]) if note else 0, int(note[1][1]) if note else 0]


class Player:
    """MainModule (:147-202) for one player.  push() is iq.push with a given id and record (what a test scripts); key_event() is
    keyEvent (:188-201) with its own IdGenerator."""

    def __init__(self, kit, base_freq):
        self.key = None                                                        # :162
        self.iq, self.next_id, self.trigger = ImpulseQueue(), 1, Trigger()     # :163-166
        self.player = SubtrackPlayer(kit, base_freq)

    def push(self, frame, note_id, freq, note_on, melody=0):
        self.iq.push(frame, note_id, (f32(freq), bool(note_on), melody))

    def key_event(self, key, down, frame, melody=0):
        """`key`: the frequency the press plays at, which also identifies the key.  -> (note_id, note_on) pushed, or None"""
        if not (down or (self.key is not None and self.key == key)):           # :190
            return None
        self.key = key if down else None                                       # :191
        note_id = self.next_id                                                 # :192 idgen.nextId()
        self.next_id += 1
        self.push(frame, note_id, key, down, melody)
        return note_id, bool(down)

    def schedule(self, out_len, sample_rate):
        """:176-185 -> (outer sub-spans, inner sub-spans in paint order)"""
        outer = self.trigger.spans(0, out_len, self.iq.consume())
        inner = []
        for s, e, (freq, on, melody), changed in outer:
            inner += self.player.paint(s, e, changed, sample_rate, freq, on, melody)
        return outer, inner

    def stats(self):
        self.player._fold_stats()
        return dict(self.player.stats)


# ---- InnerInstrument (:24-68) over the oracle's modules
DEFAULT_PATCH = (0.0, 0.025, 0.1, 0.15, 0.5)       # color :55, attack / decay / release :60-62 (cubed), sustain_volume :63
CURVE_CUBED = 3


class InnerVoice:
    """InnerInstrument's state (:33-34)"""

    def __init__(self, o):
        self.osc, self.env = o.TriSawOsc(), o.Envelope()
        o.lib().zo_trisawosc_init(C.byref(self.osc))
        o.lib().zo_envelope_init(C.byref(self.env))

    def words(self):
        e = self.env
        return [int(self.osc.cnt), bits(self.osc.t), int(e.state), bits(e.painter.t), bits(e.painter.last_value), bits(e.painter.start)]


def inner_paint(o, voice, start, end, out, temps, nic, sample_rate, freq, note_on, patch=None):
    """InnerInstrument.paint (:43-67): out, temps[0], temps[1] rows of one voice"""
    L = o.lib()
    color, attack, decay, release, sustain = patch or DEFAULT_PATCH
    L.zo_zero(start, end, o.fptr(temps[0]))                                                        # :51
    L.zo_trisawosc_paint(C.byref(voice.osc), start, end, o.fptr(temps[0]), float(sample_rate), o.constant(f32(freq)), float(color))
    L.zo_zero(start, end, o.fptr(temps[1]))                                                        # :57
    cubed = curve_cubed(o)
    ep = o.EnvelopeParams(float(sample_rate), o.curve(cubed, attack), o.curve(cubed, decay), o.curve(cubed, release), float(sustain),
                          int(bool(note_on)))
    L.zo_envelope_paint(C.byref(voice.env), start, end, o.fptr(temps[1]), int(bool(nic)), C.byref(ep))
    L.zo_multiply(start, end, o.fptr(out), o.fptr(temps[0]), o.fptr(temps[1]))                     # :66


def curve_cubed(o):
    return getattr(o, "CURVE_CUBED", CURVE_CUBED)


def render(o, voices, players_spans, frames, sample_rate, patch=None):
    """MainModule.paint into a zeroed output for every player: -> audio [N][frames]"""
    N = len(players_spans)
    audio = np.zeros((N, frames), f32)
    temps = [np.zeros(frames, f32) for _ in range(2)]
    for p, spans in enumerate(players_spans):
        for s, e, (freq, on), changed in spans:
            inner_paint(o, voices[p], s, e, audio[p], temps, changed, sample_rate, freq, on, patch)
    return audio
