"""The yardstick of the detuned-voice tests; holds no tests.  OuterInstrument.paint (examples/example_detuned.zig:125-168) and
Instrument.paint (:53-100) as the literal sequence of oracle calls -- zo_zero, zo_noise_paint, zo_filter_paint,
zo_multiply_with_scalar, zo_math_pow2f_n, zo_trisawosc_paint with a buffer cob, zo_add_into, zo_envelope_paint, zo_multiply --
per voice and per sub-span; the Trigger loop over a span table (the span paints' walk contract); and MainModule (:171-266)
composed from the host classes of zang_amd/notes.py and StereoEchoes (examples/modules.zig:464-525) as the echo tests compose it
from the oracle's delay and filtered-echoes calls.  `freq * pow(2, w)` is an np.float32 product."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests import span_reference as sr
from tests.span_reference import bits, state_words, value, walk  # noqa: F401  (state_words: for the tests)

f32 = np.float32


@dataclass
class Patch:                                       # zh_detuned_patch; the defaults are the reference's constants
    warble_hz: float = 4.0
    warble_wide: float = 4.0
    color: float = 0.0
    volume: float = 0.75
    attack: float = 0.025
    decay: float = 0.1
    release: float = 1.0
    sustain_volume: float = 0.5
    cutoff_hz: float = 880.0
    res: float = 0.8


# zh_detuned_state's words, in the struct's order: (object, field, kind), kind "q" = four u64, "f" = f32, "u" = u32
STATE = [("noise", "r", "q"), ("noise_filter", "l", "f"), ("noise_filter", "b", "f"), ("osc", "cnt", "u"), ("osc", "t", "f"),
         ("env", "state", "u"), ("env", "t", "f"), ("env", "last_value", "f"), ("env", "start", "f"),
         ("main_filter", "l", "f"), ("main_filter", "b", "f")]
# which of the 18 words are floats (compared with NaN == NaN)
FLOAT_WORDS = np.array([False] * 8 + [k == "f" for _, _, k in STATE[1:]])


class Voice:
    """OuterInstrument's modules (:113-115) with Instrument's (:41-43); `seed`: the Noise's (first_seed + v)"""

    def __init__(self, o, seed):
        L = o.lib()
        self.noise, self.noise_filter, self.osc, self.env, self.main_filter = o.Noise(), o.Filter(), o.TriSawOsc(), o.Envelope(), o.Filter()
        L.zo_noise_init(C.byref(self.noise), seed)
        L.zo_filter_init(C.byref(self.noise_filter)); L.zo_filter_init(C.byref(self.main_filter))
        L.zo_trisawosc_init(C.byref(self.osc))
        L.zo_envelope_init(C.byref(self.env))

    def words(self):
        """the state as 18 uint32 words: the generator's four u64 as (low, high), then zh_detuned_state's scalars in order"""
        out = []
        for j in range(4):
            out += [int(self.noise.r[j]) & 0xFFFFFFFF, int(self.noise.r[j]) >> 32]
        p = self.env.painter
        out += [bits(self.noise_filter.l), bits(self.noise_filter.b), int(self.osc.cnt), bits(self.osc.t), int(self.env.state), bits(p.t),
                bits(p.last_value), bits(p.start), bits(self.main_filter.l), bits(self.main_filter.b)]
        return out

    def load(self, st, v):
        """take voice v of a modules.Detuned.state() array"""
        for j in range(4):
            self.noise.r[j] = int(st["noise"]["r"][v][j])
        self.noise_filter.l, self.noise_filter.b = float(st["noise_filter"]["l"][v]), float(st["noise_filter"]["b"][v])
        self.osc.cnt, self.osc.t = int(st["osc"]["cnt"][v]), float(st["osc"]["t"][v])
        self.env.state = int(st["env"]["state"][v])
        self.env.painter.t, self.env.painter.last_value, self.env.painter.start = (float(st["env"][n][v]) for n in ("t", "last_value", "start"))
        self.main_filter.l, self.main_filter.b = float(st["main_filter"]["l"][v]), float(st["main_filter"]["b"][v])


def struct_state(st):
    """a modules.Detuned.state() array -> [V][18] uint32 words in Voice.words()'s order"""
    r = np.ascontiguousarray(st["noise"]["r"]).astype(np.uint64)                  # [V][4]
    cols = []
    for j in range(4):
        cols += [(r[:, j] & np.uint64(0xFFFFFFFF)).astype(np.uint32), (r[:, j] >> np.uint64(32)).astype(np.uint32)]
    return np.concatenate([np.stack(cols, axis=1), sr.struct_state(STATE[1:], st)], axis=1)


def same_words(a, b):
    return sr.same_words(FLOAT_WORDS, a, b)


def instrument_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, freq_warble, note_on, patch):
    """Instrument.paint (:53-100); outputs = (out0, out1 or None), temps = three rows"""
    L = o.lib()
    t0, t1, t2 = (o.fptr(t) for t in temps)
    sr, n = float(sample_rate), end - start
    if n > 0:                                                                      # :61-65
        p = np.zeros(n, f32)
        w = np.ascontiguousarray(freq_warble[start:end])
        L.zo_math_pow2f_n(o.fptr(w), o.fptr(p), n)
        with np.errstate(all="ignore"):
            temps[0][start:end] = f32(freq) * p
    L.zo_zero(start, end, t1)                                                      # :67-72
    L.zo_trisawosc_paint(C.byref(voice.osc), start, end, t1, sr, o.buffer(temps[0]), float(f32(patch.color)))
    if outputs[1] is not None:
        L.zo_add_into(start, end, o.fptr(outputs[1]), t0)                          # :74
    L.zo_multiply_with_scalar(start, end, t1, float(f32(patch.volume)))           # :76
    L.zo_zero(start, end, t0)                                                      # :78-86
    ep = o.EnvelopeParams(sr, o.curve(o.CURVE_CUBED, f32(patch.attack)), o.curve(o.CURVE_CUBED, f32(patch.decay)),
                          o.curve(o.CURVE_CUBED, f32(patch.release)), float(f32(patch.sustain_volume)), int(bool(note_on)))
    L.zo_envelope_paint(C.byref(voice.env), start, end, t0, int(bool(nic)), C.byref(ep))
    L.zo_zero(start, end, t2)                                                      # :87-88
    L.zo_multiply(start, end, t2, t1, t0)
    cut = L.zo_filter_cutoff_from_frequency(float(f32(patch.cutoff_hz)), sr)       # :90-99
    L.zo_filter_paint(C.byref(voice.main_filter), start, end, o.fptr(outputs[0]), t2, o.FILTER_LOW_PASS, o.constant(cut),
                      o.constant(float(f32(patch.res))))


def outer_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, note_on, mode, patch):
    """OuterInstrument.paint (:125-168); outputs = (out0, out1 or None), temps = four rows"""
    L = o.lib()
    t0, t1 = o.fptr(temps[0]), o.fptr(temps[1])
    sr = float(sample_rate)
    L.zo_zero(start, end, t1)                                                      # :139-140
    L.zo_noise_paint(C.byref(voice.noise), start, end, t1, o.NOISE_WHITE)
    L.zo_zero(start, end, t0)                                                      # :141-150
    cut = L.zo_filter_cutoff_from_frequency(float(f32(patch.warble_hz)), sr)
    L.zo_filter_paint(C.byref(voice.noise_filter), start, end, t0, t1, o.FILTER_LOW_PASS, o.constant(cut), o.constant(0.0))
    if (int(mode) & 1) == 0:                                                       # :152-154
        L.zo_multiply_with_scalar(start, end, t0, float(f32(patch.warble_wide)))
    instrument_paint(o, voice, start, end, outputs, temps[1:], nic, sr, freq, temps[0], note_on, patch)


FIELDS = ("freq", "note_on", "mode")


def paint_spans(o, voices, tb, img, sync, span, sample_rate, zero_first, patch, dflt=None):
    """The Trigger loop (:213-222) of every voice over its sub-spans, in place on img and sync [V][rows] (sync None: outputs[1]
    is not painted); the walk is the span paints' contract (a sub-span out of order ends the voice's list)."""
    S, E = span
    V, rows = img.shape
    temps = [np.zeros(rows, f32) for _ in range(4)]
    if zero_first:
        img[:, S:E] = 0.0
        if sync is not None:
            sync[:, S:E] = 0.0
    for v in range(V):
        for k, s, e in walk(tb, v, S, E):
            outer_paint(o, voices[v], s, e, (img[v], None if sync is None else sync[v]), temps, tb["nic"][k, v], sample_rate,
                        value(tb, dflt, "freq", k, v), int(value(tb, dflt, "note_on", k, v)) != 0, int(value(tb, dflt, "mode", k, v)), patch)
    return img


class StereoEchoes:
    """examples/modules.zig:464-525 for one voice, from the oracle's delay and filtered-echoes calls"""

    def __init__(self, o, main_delay):
        L = o.lib()
        self.o = o
        half = main_delay // 2
        self.rings = [np.zeros(half, f32), np.zeros(half, f32), np.zeros(main_delay, f32)]
        self.d0, self.d1, self.de, self.fl = o.Delay(), o.Delay(), o.Delay(), o.Filter()
        L.zo_delay_init(C.byref(self.d0), o.fptr(self.rings[0]), half)
        L.zo_delay_init(C.byref(self.d1), o.fptr(self.rings[1]), half)
        L.zo_delay_init(C.byref(self.de), o.fptr(self.rings[2]), main_delay)
        L.zo_filter_init(C.byref(self.fl))

    def paint(self, s, e, left, right, temps, x, feedback_volume, cutoff):
        o, L = self.o, self.o.lib()
        t0, t1, t2, t3 = (o.fptr(t) for t in temps)
        L.zo_add_into(s, e, o.fptr(left), o.fptr(x)); L.zo_add_into(s, e, o.fptr(right), o.fptr(x))        # :503-504
        L.zo_zero(s, e, t0); L.zo_simple_delay_paint(C.byref(self.d0), s, e, t0, o.fptr(x))               # :507-510
        L.zo_zero(s, e, t1)                                                                               # :512
        L.zo_filtered_echoes_paint(C.byref(self.de), C.byref(self.fl), s, e, t1, t2, t3, t0, float(feedback_volume), float(cutoff))   # :513-517
        L.zo_add_into(s, e, o.fptr(left), t1)                                                             # :519
        L.zo_simple_delay_paint(C.byref(self.d1), s, e, o.fptr(right), t1)                                # :520-522


class Note(C.Structure):                           # zang_amd.detuned.NOTE_PARAMS: OuterInstrument.Params without the sample rate
    _fields_ = [("freq", C.c_float), ("note_on", C.c_uint32), ("mode", C.c_uint32)]


class MainModule:
    """N players: ImpulseQueue -> Trigger per player on the host (:211-223), outer_paint per sub-span into a zeroed bus, the
    bypass of :225-230, StereoEchoes on every buffer (:232-242)"""

    def __init__(self, o, n_players, sample_rate, first_seed, main_delay, patch=None):
        from zang_amd import notes
        self.o, self.n, self.sr, self.patch = o, n_players, float(sample_rate), patch or Patch()
        ns = notes.Notes(Note)
        self.iq = [ns.ImpulseQueue() for _ in range(n_players)]
        self.tr = [notes.Trigger(Note)() for _ in range(n_players)]
        self.voices = [Voice(o, first_seed + j) for j in range(n_players)]
        self.echoes = [StereoEchoes(o, main_delay) for _ in range(n_players)]
        self.mode = 0

    def push(self, player, frame, note_id, freq, note_on):
        self.iq[player].push(frame, note_id, Note(freq, int(bool(note_on)), self.mode))       # :253-260

    def paint(self, frames):
        """-> (left, right), each [n_players][frames]"""
        from zang_amd.zang import Span
        left, right = np.zeros((self.n, frames), f32), np.zeros((self.n, frames), f32)
        temps = [np.zeros(frames, f32) for _ in range(5)]
        o, L = self.o, self.o.lib()
        for j in range(self.n):
            bus = temps[0]
            bus[:] = 0.0                                                                       # :211
            ctr = self.tr[j].counter(Span(0, frames), self.iq[j].consume())
            while True:
                r = self.tr[j].next(ctr)
                if r is None:
                    break
                q = r.params
                outer_paint(self.o, self.voices[j], r.span.start, r.span.end, (bus, None), temps[1:], r.note_id_changed, self.sr,
                            q.freq, q.note_on, q.mode, self.patch)
            if (self.mode & 2) == 0:                                                           # :225-230
                L.zo_add_into(0, frames, o.fptr(left[j]), o.fptr(bus)); L.zo_add_into(0, frames, o.fptr(right[j]), o.fptr(bus))
                L.zo_zero(0, frames, o.fptr(bus))
            self.echoes[j].paint(0, frames, left[j], right[j], temps[1:], bus, 0.6, 0.1)       # :232-242
        return left, right
