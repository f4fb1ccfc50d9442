"""The yardstick of the controlled phase-modulation voice's tests; holds no tests.  examples/example_mouse.zig and the
PhaseModOscillator of examples/modules.zig (:6-77) restated line by line in numpy f32 over the oracle's Portamento, SineOsc and
Envelope paints and basics (zo_zero, zo_set, zo_copy, zo_multiply_scalar, zo_multiply, zo_add_into), with the Trigger and
ImpulseQueue restatements the other *_reference.py files share.  PMOscInstrument.paint (:46-72) is osc_paint + instr_paint;
MainModule.paint (:148-211) is main_paint over three lists of rows (the device's tables, walked under the span paints' contract)
or, in MainModule, over three host Triggers.  The temps PERSIST across paints, as the host's do: the oscillator's temps[0] is the
instrument's temps[1] is MainModule's temps[3], `+=`-ed without being zeroed in the relative / buffer branch (modules.zig:52) and
later painted with the Envelope (example_mouse.zig:62-63).  `zero_stale` zeroes that row before each buffer: the voice's form
without a carried image."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests import span_reference as sr
from tests.span_reference import ImpulseQueue, Trigger, bits as _bits, state_words, walk  # noqa: F401  (state_words, walk: for the tests)

f32 = np.float32
CURVE_LINEAR, CURVE_CUBED = 1, 3
A4 = 440.0                                         # :22
SAMPLE_RATE = 48000                                # :8
NOTES, RATIO, MULT = 0, 1, 2                       # the three streams


@dataclass
class Patch:                                       # zh_pmctl_patch; the defaults are the reference's constants
    ctl_curve: int = CURVE_LINEAR                  # :160, :184
    ctl_glide: float = 0.1
    attack: float = 0.025                          # :65-68, cubed
    decay: float = 0.1
    release: float = 1.0
    sustain_volume: float = 0.5


class Voice:
    """one player's modules: the two controls' Portamentos (:97) and PMOscInstrument's (:36-37 over modules.zig:24-25)"""
    STATE = [("ratio", "t", "f"), ("ratio", "last_value", "f"), ("ratio", "start", "f"),
             ("multiplier", "t", "f"), ("multiplier", "last_value", "f"), ("multiplier", "start", "f"),
             ("carrier", "t", "f"), ("modulator", "t", "f"),
             ("env", "state", "u"), ("env", "t", "f"), ("env", "last_value", "f"), ("env", "start", "f")]

    def __init__(self, o):
        L = o.lib()
        self.ratio, self.multiplier = o.Portamento(), o.Portamento()
        self.carrier, self.modulator, self.env = o.SineOsc(), o.SineOsc(), o.Envelope()
        L.zo_portamento_init(C.byref(self.ratio)); L.zo_portamento_init(C.byref(self.multiplier))
        L.zo_sineosc_init(C.byref(self.carrier)); L.zo_sineosc_init(C.byref(self.modulator)); L.zo_envelope_init(C.byref(self.env))

    def words(self):
        r, m, e = self.ratio.painter, self.multiplier.painter, self.env.painter
        return [_bits(r.t), _bits(r.last_value), _bits(r.start), _bits(m.t), _bits(m.last_value), _bits(m.start),
                _bits(self.carrier.t), _bits(self.modulator.t), int(self.env.state), _bits(e.t), _bits(e.last_value), _bits(e.start)]

    def load(self, st, v):
        """take voice v of a modules.PMCtl.state() array"""
        for name, p in (("ratio", self.ratio.painter), ("multiplier", self.multiplier.painter), ("env", self.env.painter)):
            p.t, p.last_value, p.start = (float(st[name][n][v]) for n in ("t", "last_value", "start"))
        self.env.state = int(st["env"]["state"][v])
        self.carrier.t, self.modulator.t = float(st["carrier"]["t"][v]), float(st["modulator"]["t"][v])


def struct_state(st):
    """a modules.PMCtl.state() array -> [V][words] uint32 in Voice.words()'s order"""
    return sr.struct_state(Voice.STATE, st)


def same_words(a, b):
    return sr.same_words(sr.float_words(Voice.STATE), a, b)


def osc_paint(o, voice, start, end, out, temps, nic, sample_rate, freq, relative, ratio, multiplier):
    """PhaseModOscillator.paint (modules.zig:34-76): `out` its outputs[0], temps = its two rows; ratio / multiplier = ("c", value)
    or ("b", row), zang.ConstantOrBuffer.  note_id_changed reaches two SineOscs that ignore it."""
    L = o.lib()
    t0, t1 = (o.fptr(t) for t in temps)
    sr, freq = float(sample_rate), f32(freq)
    with np.errstate(all="ignore"):
        if ratio[0] == "c":                                                        # :43-49
            L.zo_set(start, end, t0, float(freq * f32(ratio[1])) if relative else float(f32(ratio[1])))
        elif relative:                                                             # :51-52: `+=` into a row nobody zeroed
            L.zo_multiply_scalar(start, end, t0, o.fptr(ratio[1]), float(freq))
        else:                                                                      # :54
            L.zo_copy(start, end, t0, o.fptr(ratio[1]))
    L.zo_zero(start, end, t1)                                                      # :58-63
    L.zo_sineosc_paint(C.byref(voice.modulator), start, end, t1, sr, o.buffer(temps[0]), o.constant(0.0))
    L.zo_zero(start, end, t0)                                                      # :64-68
    if multiplier[0] == "c":
        L.zo_multiply_scalar(start, end, t0, t1, float(f32(multiplier[1])))
    else:
        L.zo_multiply(start, end, t0, t1, o.fptr(multiplier[1]))
    L.zo_zero(start, end, t1)                                                      # :69-74
    L.zo_sineosc_paint(C.byref(voice.carrier), start, end, t1, sr, o.constant(float(freq)), o.buffer(temps[0]))
    L.zo_add_into(start, end, o.fptr(out), t1)                                     # :75


def instr_paint(o, voice, start, end, out, temps, nic, sample_rate, freq, note_on, relative, ratio, multiplier, patch):
    """PMOscInstrument.paint (example_mouse.zig:46-72); temps = three rows, [1] the carried one"""
    L = o.lib()
    sr = float(sample_rate)
    L.zo_zero(start, end, o.fptr(temps[0]))                                        # :54
    osc_paint(o, voice, start, end, temps[0], (temps[1], temps[2]), nic, sr, freq, relative, ratio, multiplier)   # :55-61
    L.zo_zero(start, end, o.fptr(temps[1]))                                        # :62
    ep = o.EnvelopeParams(sr, o.curve(o.CURVE_CUBED, f32(patch.attack)), o.curve(o.CURVE_CUBED, f32(patch.decay)),
                          o.curve(o.CURVE_CUBED, f32(patch.release)), float(f32(patch.sustain_volume)), int(bool(note_on)))
    L.zo_envelope_paint(C.byref(voice.env), start, end, o.fptr(temps[1]), int(bool(nic)), C.byref(ep))   # :63-70
    L.zo_multiply(start, end, o.fptr(out), o.fptr(temps[0]), o.fptr(temps[1]))     # :71


def control_paint(o, porta, start, end, row, nic, sample_rate, value, scale, note_on, patch):
    """one sub-span of a control (:153-168 / :177-189): goal = value * scale in f32, prev_note_on = true"""
    with np.errstate(all="ignore"):
        goal = f32(value) * f32(scale)
    o.lib().zo_portamento_paint(C.byref(porta), start, end, o.fptr(row), int(bool(nic)), float(sample_rate),
                                o.curve(int(patch.ctl_curve), f32(patch.ctl_glide)), float(goal), int(bool(note_on)), 1)


def segments(tables, v, S, E):
    """the three-cursor walk's model for one voice: the events and segments the kernel's walk makes without a wave around it
    -> [("begin", stream, k) | ("end", stream) | ("seg", f0, f1, mask)]; at one frame: ends and begins stream by stream (notes,
    ratio, multiplier), a stream's end before its next begin"""
    rows = [walk(tb, v, S, E) for tb in tables]                                    # the span paints' contract, stream by stream
    idx, active, ev = [0, 0, 0], [False, False, False], []

    def advance(i):
        for s in range(3):
            while True:
                if active[s]:
                    if rows[s][idx[s]][2] == i:
                        ev.append(("end", s)); active[s] = False; idx[s] += 1
                        continue
                    break
                if idx[s] < len(rows[s]) and rows[s][idx[s]][1] == i:
                    ev.append(("begin", s, rows[s][idx[s]][0])); active[s] = True
                    continue
                break
    i = S
    while i < E:
        advance(i)
        nxt = E
        for s in range(3):
            if active[s]:
                b = rows[s][idx[s]][2]
            else:
                b = rows[s][idx[s]][1] if idx[s] < len(rows[s]) else E
            if i < b < nxt:
                nxt = b
        ev.append(("seg", i, nxt, sum(1 << s for s in range(3) if active[s])))
        i = nxt
    advance(E)
    return ev


def main_paint(o, voice, S, E, out, temps, note_rows, ratio_rows, mult_rows, sample_rate, relative, ratio_scale, mult_scale, patch):
    """MainModule.paint (:148-211) for one player over rows [(start, end, nic, value, note_on)] per stream (notes: value = freq);
    temps = five rows that the caller keeps"""
    L = o.lib()
    L.zo_zero(S, E, o.fptr(temps[0]))                                              # :149
    for s, e, nic, value, on in ratio_rows:                                        # :151-169
        control_paint(o, voice.ratio, s, e, temps[0], nic, sample_rate, value, ratio_scale, on, patch)
    L.zo_zero(S, E, o.fptr(temps[1]))                                              # :172
    for s, e, nic, value, on in mult_rows:                                         # :175-190
        control_paint(o, voice.multiplier, s, e, temps[1], nic, sample_rate, value, mult_scale, on, patch)
    for s, e, nic, freq, on in note_rows:                                          # :193-211
        instr_paint(o, voice, s, e, out, temps[2:5], nic, sample_rate, freq, on, relative, ("b", temps[0]), ("b", temps[1]), patch)


def table_rows(tb, v, S, E, value):
    """voice v's rows of a table dict (count, start, end, nic, <value>, note_on) as main_paint takes them"""
    return [(s, e, int(tb["nic"][k, v]), tb[value][k, v], int(tb["note_on"][k, v]) != 0) for k, s, e in walk(tb, v, S, E)]


def paint_controlled(o, voices, tables, img, stale, span, sample_rate, zero_first, relative, scales, patch):
    """every voice's MainModule.paint over the three tables (notes, ratio, multiplier), in place on img [V][rows].  `stale`
    [V][rows]: each voice's carried temps[3], kept by the caller; None: zeroed before the buffer (the form without the image).
    relative and the two scales: one value, or an array per voice."""
    S, E = span
    V, rows = img.shape
    per = lambda x, v: x[v] if isinstance(x, np.ndarray) else x
    if zero_first:
        img[:, S:E] = 0.0
    for v in range(V):
        t = [np.zeros(rows, f32) for _ in range(5)]
        if stale is not None:
            t[3] = stale[v]
        main_paint(o, voices[v], S, E, img[v], t, table_rows(tables[NOTES], v, S, E, "freq"), table_rows(tables[RATIO], v, S, E, "value"),
                   table_rows(tables[MULT], v, S, E, "value"), sample_rate, bool(per(relative, v)), per(scales[0], v), per(scales[1], v), patch)
    return img


def paint_spans(o, voices, tb, img, stale, span, sample_rate, zero_first, relative, ratio, multiplier, patch, dflt=None):
    """the Trigger loop of :193-211 alone, ratio / multiplier given: ("c", value or [V]) or ("b", image [V][rows]).  A field the
    table has no array for comes from dflt (a value or [V])."""
    S, E = span
    V, rows = img.shape
    per = lambda x, v: x[v] if isinstance(x, np.ndarray) else x
    cob = lambda c, v: (c[0], per(c[1], v)) if c[0] == "c" else ("b", np.ascontiguousarray(c[1][v]))
    field = lambda name, k, v: tb[name][k, v] if tb.get(name) is not None else per(dflt[name], v)
    if zero_first:
        img[:, S:E] = 0.0
    for v in range(V):
        t = [np.zeros(rows, f32) for _ in range(3)]
        t[1] = stale[v] if stale is not None else t[1]
        for k, s, e in walk(tb, v, S, E):
            instr_paint(o, voices[v], s, e, img[v], t, int(tb["nic"][k, v]), sample_rate, field("freq", k, v), int(field("note_on", k, v)) != 0,
                        bool(per(relative, v)), cob(ratio, v), cob(multiplier, v), patch)
    return img


# ---- the example's host side
class MouseKeys:
    """keyEvent of example_mouse.zig (:230-246) for one player without the queues: key(key, down, rel_freq) -> the (freq, note_on)
    to push to the instrument's queue, or None; space() toggles the mode (:231-235)"""

    def __init__(self, a4=A4):
        self.a4, self.held, self.mode = f32(a4), None, 0

    def space(self):
        self.mode = (self.mode + 1) % 2                                            # :232

    def key(self, key, down, rel_freq):
        if not (down or self.held == key):                                         # :237
            return None
        self.held = key if down else None                                          # :238
        return f32(self.a4 * f32(rel_freq)), bool(down)                            # :239-242


class MainModule:
    """one player: three ImpulseQueue -> Trigger pairs on the host, MainModule.paint per buffer into a zeroed output.  mode_iq is
    pushed to and never consumed in the reference: not modelled."""

    def __init__(self, o, sample_rate=SAMPLE_RATE, a4=A4, patch=None, zero_stale=False):
        self.o, self.sr, self.patch, self.zero_stale = o, float(sample_rate), patch or Patch(), zero_stale
        self.keys = MouseKeys(a4)
        self.iq = [ImpulseQueue() for _ in range(3)]
        self.tr = [Trigger() for _ in range(3)]
        self.next_id = [1, 1, 1]
        self.voice = Voice(o)
        self.temps = None

    def _push(self, stream, frame, value, note_on):
        self.iq[stream].push(frame, self.next_id[stream], (f32(value), bool(note_on)))
        self.next_id[stream] += 1

    def mouse(self, x, y, frame):                                                  # :214-228
        self._push(RATIO, frame, x, True)
        self._push(MULT, frame, y, True)

    def space(self):
        self.keys.space()

    def key(self, key, down, rel_freq, frame):
        ev = self.keys.key(key, down, rel_freq)
        if ev is not None:
            self._push(NOTES, frame, ev[0], ev[1])
        return ev

    def _rows(self, stream, frames):
        out, ctr = [], self.tr[stream].counter(0, frames, self.iq[stream].consume())
        while True:
            r = self.tr[stream].next(ctr)
            if r is None:
                return out
            out.append((r[0], r[1], r[3], r[2][0], r[2][1]))

    def paint(self, frames):
        """-> audio [frames]"""
        if self.temps is None or len(self.temps[0]) < frames:
            self.temps = [np.zeros(frames, f32) for _ in range(5)]
        if self.zero_stale:
            self.temps[3][:] = 0.0
        out = np.zeros(frames, f32)
        mode = self.keys.mode                                                      # read when the buffer is painted (:161, :205)
        ratio_rows, mult_rows, note_rows = self._rows(RATIO, frames), self._rows(MULT, frames), self._rows(NOTES, frames)
        main_paint(self.o, self.voice, 0, frames, out, self.temps, note_rows, ratio_rows, mult_rows, self.sr, mode == 0,
                   4.0 if mode == 0 else 880.0, 2.0, self.patch)
        return out
