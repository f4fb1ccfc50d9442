"""The yardstick of the two-source tests; holds no tests.  examples/example_two.zig restated line by line in numpy f32, from the Zig
alone: MainModule.paint (:65-154) -- the `first` pushes, the two Triggers (src/zang/trigger.zig:26-198: tests/span_reference.py's, through `next` as the
reference has it, one sub-span per call), the merge loop of :93-151, the oracle's TriSawOsc and Envelope paints, zang.zero,
zang.multiply and zang.addScalarInto -- and keyEvent (:156-177).  The merge loop exists once (merge_loop) and runs over two `next`
callables: the Triggers' for MainModule, the rows of two tables for the stage's model (merge_table).
Where the reference is undefined: a sub-span whose end is at or below the loop's position, or above the span's end (no Trigger
makes one), ends the loop."""
import ctypes as C

import numpy as np

from tests import span_reference as sr
from tests.span_reference import ImpulseQueue, Trigger, bits, value, walk  # noqa: F401  (Trigger: for the tests)
from tests.subsong_reference import curve_cubed

f32 = np.float32
A4 = 880.0                                         # :21
SAMPLE_RATE = 48000                                # :8
DEFAULT_PATCH = (0.025, 0.1, 1.0, 0.5)             # attack / decay / release :132-134 (cubed), sustain_volume :135


def merge_loop(next0, next1, start, end):
    """:96-151 without the paints -> [(start, end, params0, params1, nic0, nic1)], one per inner span.  params_x: whatever next_x
    yields as its third element; result_x = (start, end, params, note_id_changed) or None"""
    rows = []
    r0 = next0()                                                               # :96
    r1 = next1()                                                               # :97
    while start < end:                                                         # :101
        if r0 is not None:                                                     # :103
            if r1 is not None:                                                 # :104
                inner_end = min(r0[1], r1[1])                                  # :107
                if inner_end <= start or inner_end > end:                      # undefined in the reference: ends the loop
                    break
                rows.append((start, inner_end, r0[2], r1[2], bool(r0[3]), bool(r1[3])))   # :109-138
                res0, res1 = r0, r1                                            # result0 / result1 are captures
                if res0[1] == inner_end:                                       # :139-141
                    r0 = next0()
                if res1[1] == inner_end:                                       # :142-144
                    r1 = next1()
                start = inner_end                                              # :145
                continue
        break                                                                  # :150
    return rows


def note_on_of(on0, on1):
    return bool(on0) or bool(on1)                                              # :136


def changed_of(nic0, on0, nic1, on1):
    return bool((nic0 and on0 and not nic1) or (nic1 and on1 and not nic0))   # :127-129


# ---- the stage's model: the same loop over two tables
def _rows_next(rows):
    it = iter(rows)
    return lambda: next(it, None)


def merge_player(rows_a, on_a, rows_b, on_b, out_len):
    """rows_x: [(start, end, nic, words)] of one player, words = the source's fields as uint32; on_x: the note-on field's index.
    -> [(start, end, changed, words_a + words_b + [note_on, nic_a, nic_b])]"""
    out = []
    na = _rows_next([(s, e, tuple(w), nic) for s, e, nic, w in rows_a])
    nb = _rows_next([(s, e, tuple(w), nic) for s, e, nic, w in rows_b])
    for s, e, wa, wb, nic_a, nic_b in merge_loop(na, nb, 0, out_len):
        a_on, b_on = wa[on_a] != 0, wb[on_b] != 0
        out.append((s, e, int(changed_of(nic_a, a_on, nic_b, b_on)), list(wa) + list(wb) + [int(note_on_of(a_on, b_on)), int(nic_a), int(nic_b)]))
    return out


def source_table(players_rows, n_fields, max_spans, filler_end=256):
    """a source's [span][player] table from each player's rows; rows at and above a player's count must not be read: they look
    like rows that end at `filler_end`, so that a walk that does read them makes rows no test expects"""
    N = len(players_rows)
    tb = {"count": np.zeros(N, np.uint32), "start": np.full((max_spans, N), 0xdead0001, np.uint32), "end": np.full((max_spans, N), filler_end, np.uint32),
          "nic": np.ones((max_spans, N), np.uint8), "words": np.full((n_fields, max_spans, N), 0xdead0002, np.uint32)}
    for p, rows in enumerate(players_rows):
        assert len(rows) <= max_spans
        tb["count"][p] = len(rows)
        for k, (s, e, nic, w) in enumerate(rows):
            tb["start"][k, p], tb["end"][k, p], tb["nic"][k, p] = s, e, nic
            tb["words"][:, k, p] = w
    return tb


def merge_table(players_a, on_a, players_b, on_b, out_len, max_spans, n_out):
    """the stage's table: rows at max_spans and beyond are dropped and counted.  -> (table, dropped)"""
    N = len(players_a)
    tb = {"count": np.zeros(N, np.uint32), "start": np.zeros((max_spans, N), np.uint32), "end": np.zeros((max_spans, N), np.uint32),
          "nic": np.zeros((max_spans, N), np.uint8), "words": np.zeros((n_out, max_spans, N), np.uint32)}
    dropped = 0
    for p in range(N):
        rows = merge_player(players_a[p], on_a, players_b[p], on_b, out_len)
        tb["count"][p] = min(len(rows), max_spans)
        dropped += max(0, len(rows) - max_spans)
        for k, (s, e, changed, w) in enumerate(rows[:max_spans]):
            tb["start"][k, p], tb["end"][k, p], tb["nic"][k, p] = s, e, changed
            tb["words"][:, k, p] = w
    return tb, dropped


def same_table(got, ref):
    """counts equal, and every row below a player's count equal; -> None or what differs first"""
    diff = sr.same_table(got, ref, ("start", "end", "nic"))
    if diff is not None:
        return diff
    K, live = ref["start"].shape[0], sr.live_rows(ref)
    for f in range(ref["words"].shape[0]):
        a, b = got["words"][f][:K], ref["words"][f]
        if not np.array_equal(a[live], b[live]):
            return (f"field {f}", np.argwhere((a != b) & live)[:4].tolist())
    return None


# ---- the voice (:36-37, :109-138, :153) over the oracle's modules
class Voice:
    def __init__(self, o):
        self.osc, self.env = o.TriSawOsc(), o.Envelope()
        o.lib().zo_trisawosc_init(C.byref(self.osc))                           # :52
        o.lib().zo_envelope_init(C.byref(self.env))                            # :53

    def words(self):
        """zh_dual_state's six words"""
        e = self.env
        return [int(self.osc.cnt), bits(self.osc.t), int(e.state), bits(e.painter.t), bits(e.painter.last_value), bits(e.painter.start)]


def inner_span_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, color, note_on, patch=None):
    """:109-138 for one inner span: outputs[1] (or None), temps[0] and temps[1] rows of one voice"""
    L = o.lib()
    attack, decay, release, sustain = patch or DEFAULT_PATCH
    if outputs[1] is not None:
        L.zo_add_scalar_into(start, end, o.fptr(outputs[1]), float(f32(freq)))       # :109
    L.zo_trisawosc_paint(C.byref(voice.osc), start, end, o.fptr(temps[0]), float(sample_rate), o.constant(f32(freq)), float(f32(color)))   # :110-120
    cubed = curve_cubed(o)
    ep = o.EnvelopeParams(float(sample_rate), o.curve(cubed, attack), o.curve(cubed, decay), o.curve(cubed, release), float(sustain),
                          int(bool(note_on)))
    L.zo_envelope_paint(C.byref(voice.env), start, end, o.fptr(temps[1]), int(bool(nic)), C.byref(ep))   # :121-138


def sub_span_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, color, note_on, patch=None):
    """what the span paint does over ONE sub-span: the zeros of :83-84, the inner span, the multiply of :153, all over [start, end)"""
    L = o.lib()
    L.zo_zero(start, end, o.fptr(temps[0]))
    L.zo_zero(start, end, o.fptr(temps[1]))
    inner_span_paint(o, voice, start, end, outputs, temps, nic, sample_rate, freq, color, note_on, patch)
    L.zo_multiply(start, end, o.fptr(outputs[0]), o.fptr(temps[0]), o.fptr(temps[1]))


FIELDS = ("freq", "color", "note_on")


def paint_spans(o, voices, tb, img, sync, span, sample_rate, zero_first, patch=None, dflt=None):
    """the span paint's contract for every voice over its sub-spans, in place on img and sync [V][rows] (sync None: outputs[1] is
    not painted); a sub-span out of order ends the voice's list; frames no sub-span covers are left alone"""
    S, E = span
    V, rows = img.shape
    temps = [np.zeros(rows, f32) for _ in range(2)]
    if zero_first:
        img[:, S:E] = 0.0
        if sync is not None:
            sync[:, S:E] = 0.0
    for v in range(V):
        for k, s, e in walk(tb, v, S, E):
            sub_span_paint(o, voices[v], s, e, (img[v], None if sync is None else sync[v]), temps, tb["nic"][k, v], sample_rate,
                           value(tb, dflt, "freq", k, v), value(tb, dflt, "color", k, v), int(value(tb, dflt, "note_on", k, v)) != 0, patch)
    return img


# ---- MainModule (:23-178) for one player
class MainModule:
    def __init__(self, o, a4=A4, sample_rate=SAMPLE_RATE):
        self.o, self.a4, self.sample_rate = o, f32(a4), float(sample_rate)
        self.first = True                                                      # :51
        self.voice = Voice(o)                                                  # :52-53
        self.key0, self.iq0, self.next_id0, self.trig0 = None, ImpulseQueue(), 1, Trigger()   # :54-57
        self.key1, self.iq1, self.next_id1, self.trig1 = None, ImpulseQueue(), 1, Trigger()   # :58-61
        self.rows = []                                                         # the last paint's inner spans

    def _id0(self):
        self.next_id0 += 1
        return self.next_id0 - 1

    def _id1(self):
        self.next_id1 += 1
        return self.next_id1 - 1

    def _first(self):
        """:71-81.  The reference makes these pushes in its first paint; a key event before that paint would then stand in the
        queue first, and a frame-0 push behind a later frame is refused (notes.zig:112-118).  The device player makes them at
        construction, before any key, and so does this model: at the first key event or paint, whichever comes first."""
        if self.first:
            self.first = False
            self.iq0.push(0, self._id0(), (f32(self.a4 * f32(0.5)), False))
            self.iq1.push(0, self._id1(), (f32(0.5), False))

    def key_event(self, key, down, frame, rel_freq=None, number=None):
        """:156-177.  `rel_freq`: what getKeyRelFreqFromRow(0, key) gives, or None; `number`: key - SDLK_1 for a number key (0..8),
        or None.  The `first` pushes draw id 1 of each generator whenever they happen: a key's ids start at 2."""
        self._first()
        if rel_freq is not None:                                               # :157
            if down or (self.key0 is not None and self.key0 == key):           # :158
                self.key0 = key if down else None                              # :159
                self.iq0.push(frame, self._id0(), (f32(self.a4 * f32(rel_freq)), bool(down)))   # :160-163
        if number is not None:                                                 # :166
            f = f32(number) / f32(8)                                           # :167
            if down or (self.key1 is not None and self.key1 == key):           # :168
                self.key1 = key if down else None                              # :169
                color = f32(0.5) + np.sqrt(f, dtype=f32) * f32(0.5)            # :171
                self.iq1.push(frame, self._id1(), (f32(color), bool(down)))

    def paint(self, frames, outputs, temps):
        """:65-154 over span = [0, frames): outputs = (audio row, sync row), temps = two rows"""
        o, L = self.o, self.o.lib()
        self._first()                                                          # :71-81
        L.zo_zero(0, frames, o.fptr(temps[0]))                                 # :83
        L.zo_zero(0, frames, o.fptr(temps[1]))                                 # :84
        ctr0 = self.trig0.counter(0, frames, self.iq0.consume())               # :93
        ctr1 = self.trig1.counter(0, frames, self.iq1.consume())               # :94
        # the paints touch no Trigger: the loop is run first, then its inner spans are painted in order
        self.rows = merge_loop(lambda: self.trig0.next(ctr0), lambda: self.trig1.next(ctr1), 0, frames)
        for s, e, (freq, on0), (color, on1), nic0, nic1 in self.rows:
            inner_span_paint(o, self.voice, s, e, outputs, temps, changed_of(nic0, on0, nic1, on1), self.sample_rate, freq, color,
                             note_on_of(on0, on1))
        L.zo_multiply(0, frames, o.fptr(outputs[0]), o.fptr(temps[0]), o.fptr(temps[1]))   # :153
