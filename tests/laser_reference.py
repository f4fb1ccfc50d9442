"""The yardstick of the laser tests; holds no tests.  LaserPlayer.paint (examples/example_laser.zig:67-116) as the literal
sequence of oracle calls -- zo_zero, zo_curve_paint, zo_multiply_with_scalar, zo_sineosc_paint with buffer cobs, zo_multiply --
per voice and per sub-span; the Trigger loop over a span table (the span paints' walk contract); and MainModule (:119-159)
composed from the host classes of zang_amd/notes.py.  The product of two scalars is an np.float32 product.

A kit is what zang_amd.sfx.SfxKit takes: a list of (modulator, carrier, volume), each ([(t, value), ...], function).  Its node
array is restated here as the library lays it out (all nodes in order, then as many zero nodes as the longest curve has): a
Curve reads the node it carried over at the index its last paint left, counted from the first node of the curve it plays now."""
import ctypes as C

import numpy as np

from tests import span_reference as sr
from tests.span_reference import state_words, value, walk  # noqa: F401  (state_words: for the tests)

f32 = np.float32


class Kit:
    def __init__(self, effects):
        rows, self.desc = [], []
        longest = 0
        for triple in effects:
            d = []
            for curve, function in triple:
                d.append((len(rows), len(curve), int(function)))
                rows += [(value, t) for t, value in curve]
                longest = max(longest, len(curve))
            self.desc.append(d)
        rows += [(0.0, 0.0)] * longest
        self.nodes = np.array(rows, f32).reshape(-1, 2)              # {value, t}
        self.count = len(effects)

    def curve(self, o, effect, which):
        """-> (pointer to the curve's first node, count, function, offset)"""
        off, n, fn = self.desc[effect][which]
        return C.cast(self.nodes.ctypes.data + 8 * off, C.POINTER(o.CurveNode)), n, fn, off


class Voice:
    """LaserPlayer's five modules (:51-55)"""

    def __init__(self, o):
        L = o.lib()
        self.carrier_curve, self.modulator_curve, self.volume_curve = o.CurveModule(), o.CurveModule(), o.CurveModule()
        self.carrier, self.modulator = o.SineOsc(), o.SineOsc()
        for c in (self.carrier_curve, self.modulator_curve, self.volume_curve):
            L.zo_curve_init(C.byref(c))
        for s in (self.carrier, self.modulator):
            L.zo_sineosc_init(C.byref(s))

    STATE = [("carrier_curve", "t"), ("carrier_curve", "current_song_note"), ("carrier_curve", "current_song_note_offset"),
             ("carrier_curve", "next_song_note"), ("carrier", "t"), ("modulator_curve", "t"), ("modulator_curve", "current_song_note"),
             ("modulator_curve", "current_song_note_offset"), ("modulator_curve", "next_song_note"), ("modulator", "t"),
             ("volume_curve", "t"), ("volume_curve", "current_song_note"), ("volume_curve", "current_song_note_offset"),
             ("volume_curve", "next_song_note")]

    def words(self):
        """the state as zh_laser_state's 14 words (uint32 bits)"""
        out = []
        for obj, field in self.STATE:
            x = getattr(getattr(self, obj), field)
            out.append(int(np.array([x], f32).view(np.uint32)[0]) if field == "t" else int(x) & 0xFFFFFFFF)
        return out


def struct_state(st):
    """a modules.Laser.state() array -> [V][14] uint32 words in the same order"""
    return sr.struct_state(Voice.STATE, st)


def laser_paint(o, voice, kit, start, end, out, temps, nic, sample_rate, freq_mul, carrier_mul, modulator_mul, modulator_rad, effect):
    """LaserPlayer.paint (:67-116) on one voice's row `out` with three temp rows.  effect >= kit.count: nothing at all."""
    if effect >= kit.count:
        return
    L = o.lib()
    t0, t1, t2 = (o.fptr(t) for t in temps)
    nic, sr = int(bool(nic)), float(sample_rate)

    def curve(state, dest, which):
        ptr, n, fn, off = kit.curve(o, effect, which)
        if not nic and state.current_song_note < state.next_song_note and off + state.current_song_note >= len(kit.nodes):
            state.current_song_note = state.next_song_note            # (a set_state index past the kit's array: dropped)
        L.zo_curve_paint(C.byref(state), start, end, dest, nic, sr, fn, ptr, n)

    L.zo_zero(start, end, t0)
    curve(voice.modulator_curve, t0, 0)
    L.zo_multiply_with_scalar(start, end, t0, float(f32(freq_mul) * f32(modulator_mul)))
    L.zo_zero(start, end, t1)
    L.zo_sineosc_paint(C.byref(voice.modulator), start, end, t1, sr, o.buffer(temps[0]), o.constant(0.0))
    L.zo_multiply_with_scalar(start, end, t1, float(f32(modulator_rad)))
    L.zo_zero(start, end, t0)
    curve(voice.carrier_curve, t0, 1)
    L.zo_multiply_with_scalar(start, end, t0, float(f32(freq_mul) * f32(carrier_mul)))
    L.zo_zero(start, end, t2)
    L.zo_sineosc_paint(C.byref(voice.carrier), start, end, t2, sr, o.buffer(temps[0]), o.buffer(temps[1]))
    L.zo_zero(start, end, t0)
    curve(voice.volume_curve, t0, 2)
    L.zo_multiply(start, end, o.fptr(out), t0, t2)


FIELDS = ("freq_mul", "carrier_mul", "modulator_mul", "modulator_rad", "effect")


def paint_spans(o, kit, voices, tb, img, span, sample_rate, zero_first, dflt=None):
    """The Trigger loop (:149-158) of every voice over its sub-spans, in place on img [V][rows]; the walk is the span paints'
    contract (a sub-span out of order ends the voice's list)."""
    S, E = span
    V, rows = img.shape
    temps = [np.zeros(rows, f32) for _ in range(3)]
    if zero_first:
        img[:, S:E] = 0.0
    for v in range(V):
        for k, s, e in walk(tb, v, S, E):
            laser_paint(o, voices[v], kit, s, e, img[v], temps, tb["nic"][k, v], sample_rate,
                        *(value(tb, dflt, n, k, v) for n in FIELDS[:4]), int(value(tb, dflt, "effect", k, v)))
    return img


class Note(C.Structure):                           # zang_amd.sfx.NOTE_PARAMS
    _fields_ = [("freq_mul", C.c_float), ("carrier_mul", C.c_float), ("modulator_mul", C.c_float), ("modulator_rad", C.c_float),
                ("effect", C.c_uint32), ("note_on", C.c_uint32)]


class MainModule:
    """N players of `polyphony` voices: ImpulseQueue -> PolyphonyDispatcher -> Trigger per player on the host, laser_paint per
    sub-span, each voice into its own row (polyphony 1: the player's row)"""

    def __init__(self, o, kit, n_players, polyphony, sample_rate):
        from zang_amd import notes
        self.o, self.kit, self.n, self.p, self.sr = o, kit, n_players, polyphony, float(sample_rate)
        ns = notes.Notes(Note)
        self.iq = [ns.ImpulseQueue() for _ in range(n_players)]
        self.pd = [ns.PolyphonyDispatcher(polyphony)() for _ in range(n_players)]
        self.tr = [[notes.Trigger(Note)() for _ in range(polyphony)] for _ in range(n_players)]
        self.voices = [[Voice(o) for _ in range(polyphony)] for _ in range(n_players)]

    def push(self, player, frame, note_id, effect, freq_mul, carrier_mul, modulator_mul, modulator_rad):
        self.iq[player].push(frame, note_id, Note(freq_mul, carrier_mul, modulator_mul, modulator_rad, effect, 1))

    def paint(self, frames):
        """-> [n_players * polyphony][frames], one row per voice"""
        from zang_amd.zang import Span
        out = np.zeros((self.n * self.p, frames), f32)
        temps = [np.zeros(frames, f32) for _ in range(3)]
        for j in range(self.n):
            poly = self.pd[j].dispatch(self.iq[j].consume())
            for i in range(self.p):
                ctr = self.tr[j][i].counter(Span(0, frames), poly[i])
                while True:
                    r = self.tr[j][i].next(ctr)
                    if r is None:
                        break
                    q = r.params
                    laser_paint(self.o, self.voices[j][i], self.kit, r.span.start, r.span.end, out[j * self.p + i], temps, r.note_id_changed,
                                self.sr, q.freq_mul, q.carrier_mul, q.modulator_mul, q.modulator_rad, q.effect)
        return out
