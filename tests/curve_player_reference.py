"""The yardstick of the curve-voice tests; holds no tests.  CurvePlayer.paint (examples/example_curve.zig:55-95) as the literal
sequence of oracle calls -- zo_zero, zo_curve_paint, zo_multiply_with_scalar, zo_sineosc_paint with buffer cobs, zo_add_into --
per voice and per sub-span; the Trigger loop over a span table (the span paints' walk contract) over TWO rows per voice, the
voice's and its frequency image's; and MainModule (:98-144) composed from the host classes of zang_amd/notes.py.

A kit is tests/laser_reference.Kit: what zang_amd.sfx.SfxKit takes, its node array restated as the library lays it out.  The
voice plays an effect's modulator (0) and carrier (1) curves and never looks at the volume curve."""
import ctypes as C

import numpy as np

from tests import span_reference as sr
from tests.laser_reference import Kit  # noqa: F401  (re-exported for the tests)
from tests.span_reference import state_words, value, walk  # noqa: F401  (state_words: for the tests)

f32 = np.float32


class Voice:
    """CurvePlayer's four modules (:41-44)"""

    def __init__(self, o):
        L = o.lib()
        self.carrier_curve, self.modulator_curve = o.CurveModule(), o.CurveModule()
        self.carrier, self.modulator = o.SineOsc(), o.SineOsc()
        for c in (self.carrier_curve, self.modulator_curve):
            L.zo_curve_init(C.byref(c))
        for s in (self.carrier, self.modulator):
            L.zo_sineosc_init(C.byref(s))

    STATE = [("carrier_curve", "t"), ("carrier_curve", "current_song_note"), ("carrier_curve", "current_song_note_offset"),
             ("carrier_curve", "next_song_note"), ("carrier", "t"), ("modulator_curve", "t"), ("modulator_curve", "current_song_note"),
             ("modulator_curve", "current_song_note_offset"), ("modulator_curve", "next_song_note"), ("modulator", "t")]

    def words(self):
        """the state as zh_curve_player_state's 10 words (uint32 bits)"""
        out = []
        for obj, field in self.STATE:
            x = getattr(getattr(self, obj), field)
            out.append(int(np.array([x], f32).view(np.uint32)[0]) if field == "t" else int(x) & 0xFFFFFFFF)
        return out


def struct_state(st):
    """a modules.CurveVoice.state() array -> [V][10] uint32 words in the same order"""
    return sr.struct_state(Voice.STATE, st)


def curve_player_paint(o, voice, kit, start, end, out0, out1, temps, nic, sample_rate, rel_freq, effect):
    """CurvePlayer.paint (:55-95) on one voice's rows `out0` and `out1` (None: the reference's outputs[1] goes to a row nobody
    reads) with two temp rows.  effect >= kit.count: nothing at all."""
    if effect >= kit.count:
        return
    L = o.lib()
    t0, t1 = (o.fptr(t) for t in temps)
    nic, sr, mul = int(bool(nic)), float(sample_rate), float(f32(rel_freq))

    def curve(state, dest, which):
        ptr, n, fn, off = kit.curve(o, effect, which)
        if not nic and state.current_song_note < state.next_song_note and off + state.current_song_note >= len(kit.nodes):
            state.current_song_note = state.next_song_note            # (a set_state index past the kit's array: dropped)
        L.zo_curve_paint(C.byref(state), start, end, dest, nic, sr, fn, ptr, n)

    L.zo_zero(start, end, t0)                                         # :65
    curve(voice.modulator_curve, t0, 0)                               # :66-70
    L.zo_multiply_with_scalar(start, end, t0, mul)                    # :71
    L.zo_zero(start, end, t1)                                         # :73
    L.zo_sineosc_paint(C.byref(voice.modulator), start, end, t1, sr, o.buffer(temps[0]), o.constant(0.0))        # :74-78
    L.zo_zero(start, end, t0)                                         # :80
    curve(voice.carrier_curve, t0, 1)                                 # :81-85
    L.zo_multiply_with_scalar(start, end, t0, mul)                    # :86
    L.zo_sineosc_paint(C.byref(voice.carrier), start, end, o.fptr(out0), sr, o.buffer(temps[0]), o.buffer(temps[1]))   # :88-92
    if out1 is not None:
        L.zo_add_into(start, end, o.fptr(out1), t0)                   # :94


FIELDS = ("rel_freq", "effect")


def paint_spans(o, kit, voices, tb, img0, img1, span, sample_rate, zero_first, dflt=None):
    """The Trigger loop (:126-129) of every voice over its sub-spans, in place on img0 and img1 [V][rows] (img1 None: no frequency
    image); the walk is the span paints' contract (a sub-span out of order ends the voice's list)."""
    S, E = span
    V, rows = img0.shape
    temps = [np.zeros(rows, f32) for _ in range(2)]
    if zero_first:
        img0[:, S:E] = 0.0
        if img1 is not None:
            img1[:, S:E] = 0.0
    for v in range(V):
        for k, s, e in walk(tb, v, S, E):
            curve_player_paint(o, voices[v], kit, s, e, img0[v], None if img1 is None else img1[v], temps, tb["nic"][k, v], sample_rate,
                               value(tb, dflt, "rel_freq", k, v), int(value(tb, dflt, "effect", k, v)))
    return img0, img1


class Note(C.Structure):                           # zang_amd.sfx.CURVE_NOTE_PARAMS
    _fields_ = [("rel_freq", C.c_float), ("effect", C.c_uint32), ("note_on", C.c_uint32)]


class MainModule:
    """N players of `polyphony` voices: ImpulseQueue -> PolyphonyDispatcher -> Trigger per player on the host, curve_player_paint
    per sub-span, each voice into its own rows (polyphony 1: the player's)"""

    def __init__(self, o, kit, n_players, polyphony, sample_rate):
        from zang_amd import notes
        self.o, self.kit, self.n, self.p, self.sr = o, kit, n_players, polyphony, float(sample_rate)
        ns = notes.Notes(Note)
        self.iq = [ns.ImpulseQueue() for _ in range(n_players)]
        self.pd = [ns.PolyphonyDispatcher(polyphony)() for _ in range(n_players)]
        self.tr = [[notes.Trigger(Note)() for _ in range(polyphony)] for _ in range(n_players)]
        self.voices = [[Voice(o) for _ in range(polyphony)] for _ in range(n_players)]

    def push(self, player, frame, note_id, effect, rel_freq):
        self.iq[player].push(frame, note_id, Note(rel_freq, effect, 1))

    def paint(self, frames):
        """-> (voices, frequency images), each [n_players * polyphony][frames], one row per voice"""
        from zang_amd.zang import Span
        out0, out1 = (np.zeros((self.n * self.p, frames), f32) for _ in range(2))
        temps = [np.zeros(frames, f32) for _ in range(2)]
        for j in range(self.n):
            poly = self.pd[j].dispatch(self.iq[j].consume())
            for i in range(self.p):
                ctr = self.tr[j][i].counter(Span(0, frames), poly[i])
                while True:
                    r = self.tr[j][i].next(ctr)
                    if r is None:
                        break
                    q = r.params
                    row = j * self.p + i
                    curve_player_paint(self.o, self.voices[j][i], self.kit, r.span.start, r.span.end, out0[row], out1[row], temps,
                                       r.note_id_changed, self.sr, q.rel_freq, q.effect)
        return out0, out1
