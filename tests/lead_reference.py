"""The yardstick of the lead-voice tests; holds no tests.  Instrument.paint of examples/example_portamento.zig (:43-86) and of
examples/example_vibrato.zig (:38-68) as the literal sequence of oracle calls -- zo_zero, zo_portamento_paint, zo_envelope_paint,
zo_sineosc_paint with a buffer cob, zo_multiply, zo_add_into; zo_sineosc_paint, zo_pulseosc_paint with a buffer cob, zo_gate_paint,
zo_multiply -- per voice and per sub-span; the Trigger loop over a span table (the span paints' walk contract); both MainModules
composed from the host classes of zang_amd/notes.py; keyEvent of the portamento example (:135-173) restated.  prev_note_on is
carried here; `freq * (1 + depth * m)` is three np.float32 operations."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests import span_reference as sr
from tests.span_reference import bits as _bits, state_words, value, walk  # noqa: F401  (state_words: for the tests)

f32 = np.float32
CURVE_CUBED = 3


@dataclass
class PortaPatch:                                  # zh_porta_patch; the defaults are the reference's constants
    glide_curve: int = CURVE_CUBED
    glide: float = 0.5
    attack: float = 0.025
    decay: float = 0.1
    release: float = 1.0
    sustain_volume: float = 0.5


@dataclass
class VibratoPatch:                                # zh_vibrato_patch
    vib_hz: float = 4.0
    depth: float = 0.02
    color: float = 0.5


class PortaVoice:
    """Instrument's modules and prev_note_on (:29-32)"""
    STATE = [("porta", "t", "f"), ("porta", "last_value", "f"), ("porta", "start", "f"), ("env", "state", "u"), ("env", "t", "f"),
             ("env", "last_value", "f"), ("env", "start", "f"), ("osc", "t", "f"), (None, "prev_note_on", "u")]

    def __init__(self, o):
        L = o.lib()
        self.porta, self.env, self.osc, self.prev_note_on = o.Portamento(), o.Envelope(), o.SineOsc(), False
        L.zo_portamento_init(C.byref(self.porta)); L.zo_envelope_init(C.byref(self.env)); L.zo_sineosc_init(C.byref(self.osc))

    def words(self):
        p, e = self.porta.painter, self.env.painter
        return [_bits(p.t), _bits(p.last_value), _bits(p.start), int(self.env.state), _bits(e.t), _bits(e.last_value), _bits(e.start),
                _bits(self.osc.t), int(self.prev_note_on)]

    def load(self, st, v):
        """take voice v of a modules.Porta.state() array"""
        p, e = self.porta.painter, self.env.painter
        p.t, p.last_value, p.start = (float(st["porta"][n][v]) for n in ("t", "last_value", "start"))
        self.env.state = int(st["env"]["state"][v])
        e.t, e.last_value, e.start = (float(st["env"][n][v]) for n in ("t", "last_value", "start"))
        self.osc.t = float(st["osc"]["t"][v])
        self.prev_note_on = bool(st["prev_note_on"][v])


class VibratoVoice:
    """Instrument's modules (:26-28); the Gate has no state"""
    STATE = [("vib", "t", "f"), ("osc", "cnt", "u")]

    def __init__(self, o):
        L = o.lib()
        self.vib, self.osc = o.SineOsc(), o.PulseOsc()
        L.zo_sineosc_init(C.byref(self.vib)); L.zo_pulseosc_init(C.byref(self.osc))

    def words(self):
        return [_bits(self.vib.t), int(self.osc.cnt)]

    def load(self, st, v):
        self.vib.t, self.osc.cnt = float(st["vib"]["t"][v]), int(st["osc"]["cnt"][v])


def struct_state(cls, st):
    """a modules.Porta / Vibrato .state() array -> [V][words] uint32 in cls.words()'s order"""
    return sr.struct_state(cls.STATE, st)


def same_words(cls, a, b):
    return sr.same_words(sr.float_words(cls.STATE), a, b)


def porta_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, note_on, patch):
    """Instrument.paint of example_portamento.zig (:43-86); outputs = (out0, out1 or None), temps = three rows"""
    L = o.lib()
    t0, t1, t2 = (o.fptr(t) for t in temps)
    sr, note_on, prev = float(sample_rate), bool(note_on), bool(voice.prev_note_on)
    L.zo_zero(start, end, t0)                                                      # :53-61
    L.zo_portamento_paint(C.byref(voice.porta), start, end, t0, int(bool(nic)), sr, o.curve(int(patch.glide_curve), f32(patch.glide)),
                          float(f32(freq)), int(note_on), int(prev))
    L.zo_zero(start, end, t1)                                                      # :63-73
    ep = o.EnvelopeParams(sr, o.curve(o.CURVE_CUBED, f32(patch.attack)), o.curve(o.CURVE_CUBED, f32(patch.decay)),
                          o.curve(o.CURVE_CUBED, f32(patch.release)), float(f32(patch.sustain_volume)), int(note_on))
    L.zo_envelope_paint(C.byref(voice.env), start, end, t1, int((not prev) and note_on), C.byref(ep))
    L.zo_zero(start, end, t2)                                                      # :75-80
    L.zo_sineosc_paint(C.byref(voice.osc), start, end, t2, sr, o.buffer(temps[0]), o.constant(0.0))
    L.zo_multiply(start, end, o.fptr(outputs[0]), t1, t2)                          # :82
    if outputs[1] is not None:
        L.zo_add_into(start, end, o.fptr(outputs[1]), t0)                          # :85
    voice.prev_note_on = note_on                                                   # the defer of :51


def vibrato_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, note_on, patch):
    """Instrument.paint of example_vibrato.zig (:38-68); note_id_changed reaches modules that ignore it"""
    L = o.lib()
    t0, t1, t2 = (o.fptr(t) for t in temps)
    sr = float(sample_rate)
    L.zo_zero(start, end, t2)                                                      # :46-51
    L.zo_sineosc_paint(C.byref(voice.vib), start, end, t2, sr, o.constant(float(f32(patch.vib_hz))), o.constant(0.0))
    with np.errstate(all="ignore"):                                                # :52-55
        dm = f32(patch.depth) * temps[2][start:end]
        one = f32(1.0) + dm
        temps[2][start:end] = f32(freq) * one
    if outputs[1] is not None:
        L.zo_add_into(start, end, o.fptr(outputs[1]), t2)                          # :56
    L.zo_zero(start, end, t0)                                                      # :57-62
    L.zo_pulseosc_paint(C.byref(voice.osc), start, end, t0, sr, o.buffer(temps[2]), float(f32(patch.color)))
    L.zo_zero(start, end, t1)                                                      # :63-66
    L.zo_gate_paint(start, end, t1, int(bool(note_on)))
    L.zo_multiply(start, end, o.fptr(outputs[0]), t0, t1)                          # :67


FIELDS = ("freq", "note_on")


def paint_spans(o, paint, voices, tb, img, sync, span, sample_rate, zero_first, patch, dflt=None):
    """The Trigger loop of every voice over its sub-spans, in place on img and sync [V][rows] (sync None: outputs[1] is not
    painted); `paint` = porta_paint or vibrato_paint; the walk is the span paints' contract (a sub-span out of order ends the
    voice's list)."""
    S, E = span
    V, rows = img.shape
    temps = [np.zeros(rows, f32) for _ in range(3)]
    if zero_first:
        img[:, S:E] = 0.0
        if sync is not None:
            sync[:, S:E] = 0.0
    for v in range(V):
        for k, s, e in walk(tb, v, S, E):
            paint(o, voices[v], s, e, (img[v], None if sync is None else sync[v]), temps, tb["nic"][k, v], sample_rate,
                  value(tb, dflt, "freq", k, v), int(value(tb, dflt, "note_on", k, v)) != 0, patch)
    return img


class Note(C.Structure):                           # zang_amd.lead.NOTE_PARAMS: Instrument.Params without the sample rate
    _fields_ = [("freq", C.c_float), ("note_on", C.c_uint32)]


class MainModule:
    """N players: ImpulseQueue -> Trigger per player on the host, Instrument.paint per sub-span into zeroed outputs (portamento
    :113-129, vibrato :95-111); `voice_cls`, `paint`: the voice"""

    def __init__(self, o, voice_cls, paint, n_players, sample_rate, patch):
        from zang_amd import notes
        self.o, self.n, self.sr, self.patch, self.paint_voice = o, n_players, float(sample_rate), patch, paint
        ns = notes.Notes(Note)
        self.iq = [ns.ImpulseQueue() for _ in range(n_players)]
        self.tr = [notes.Trigger(Note)() for _ in range(n_players)]
        self.voices = [voice_cls(o) for _ in range(n_players)]

    def push(self, player, frame, note_id, freq, note_on):
        self.iq[player].push(frame, note_id, Note(freq, int(bool(note_on))))

    def paint(self, frames):
        """-> (audio, sync), each [n_players][frames]"""
        from zang_amd.zang import Span
        audio, sync = np.zeros((self.n, frames), f32), np.zeros((self.n, frames), f32)
        temps = [np.zeros(frames, f32) for _ in range(3)]
        for j in range(self.n):
            ctr = self.tr[j].counter(Span(0, frames), self.iq[j].consume())
            while True:
                r = self.tr[j].next(ctr)
                if r is None:
                    break
                q = r.params
                self.paint_voice(self.o, self.voices[j], r.span.start, r.span.end, (audio[j], sync[j]), temps, r.note_id_changed, self.sr,
                                 q.freq, q.note_on, self.patch)
        return audio, sync


class PortaKeys:
    """keyEvent of example_portamento.zig (:135-173) for one player, restated: -> the (note_id, freq, note_on) it pushes, or None.
    `key_freqs[i]` stands for a4 * key_bindings[i].rel_freq; ids come from an IdGenerator that starts at 1."""

    def __init__(self, key_freqs):
        self.key_freqs, self.keys_held, self.next_id = list(key_freqs), 0, 1

    def _id(self):
        i = self.next_id
        self.next_id += 1
        return i

    def key_event(self, key_index, down):
        flag = 1 << key_index
        prev = self.keys_held
        if down:
            self.keys_held |= flag                                                 # :146
            if flag > prev:                                                        # :148
                return (self._id(), self.key_freqs[key_index], True)
            return None
        self.keys_held &= ~flag                                                    # :156
        if self.keys_held == 0:                                                    # :158-163
            return (self._id(), self.key_freqs[key_index], False)
        top = self.keys_held.bit_length() - 1                                      # 63 - clz (:165)
        return (self._id(), self.key_freqs[top], True)
