"""TwoPlayer: N of the reference's two-source example played live (examples/example_two.zig MainModule :23-178): one voice
driven by two impulse streams -- keys set the frequency, number keys the oscillator's colour, either triggers the envelope.  Per
buffer: each source's pushed records go through one LiveVoiceBank launch (the two ImpulseQueue -> Trigger pairs, :93-97; polyphony
1), one merge-stage launch cuts the two tables into one (the loop of :101-151, zh_span_merge_schedule) and one Dual span paint with
zero-first renders it into the audio image and the frequency image (:109-138, :153).  Nothing runs on the host per player."""
import ctypes as C

import numpy as np

from . import abi, modules as mod, zang
from .bank import LiveVoiceBank
from .stage import Stage, StageTable

# the sources' records: Params0 / Params1 (:31-32), and a word that is always set for the bank's dispatcher (every push takes slot
# 0, note-offs included: the bare Triggers of MainModule.paint)
FREQ_PARAMS = np.dtype([("freq", "<f4"), ("note_on", "<u4"), ("on", "<u4")])
COLOR_PARAMS = np.dtype([("color", "<f4"), ("note_on", "<u4"), ("on", "<u4")])
SOURCE_SPANS = 34                               # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
MAX_SPANS = 67                                  # what two SOURCE_SPANS-row tables can make
A4 = 880.0                                      # :21


MergeTable = StageTable


def _source(fields, on):
    names = [n for n, _ in fields]
    d = abi.SpanMergeSource(len(fields), names.index(on) if on in names else len(fields))
    for i, (_, kind) in enumerate(fields[:abi.SPAN_MERGE_MAX_FIELDS]):
        d.kinds[i] = ord(kind)
    return d


class SpanMerge(Stage):
    """zh_span_merge_*: the loop of examples/example_two.zig:93-151 for n players, without the voice.  `fields_a` / `fields_b`: 1 to 4
    (name, "f" or "u") per source, the names those of the stage's output fields; `on_a` / `on_b`: the name of each source's note-on
    field (kind "u").  The output's fields: A's, then B's, then "note_on" (on_a | on_b), "nic_a" and "nic_b"; its note_id_changed
    is (nic_a & on_a & !nic_b) | (nic_b & on_b & !nic_a).  A source's nic stays set on every row cut from the same source row;
    the sources' starts are never read; nothing follows once either source has no row left.  The stage keeps no state.  The table
    has 67 rows at creation; download() gives every field as uint32 words."""
    PREFIX = "zh_span_merge"

    def __init__(self, ctx, n_players, fields_a, on_a, fields_b, on_b, rows=None):
        self.fields_a, self.fields_b = list(fields_a), list(fields_b)
        self.names = [n for n, _ in self.fields_a] + [n for n, _ in self.fields_b] + ["note_on", "nic_a", "nic_b"]
        if len(set(self.names)) != len(self.names):
            raise ValueError("field names must differ (and from note_on, nic_a, nic_b)")
        self.FIELDS = [(name, field) for field, name in enumerate(self.names)]
        a, b = _source(self.fields_a, on_a), _source(self.fields_b, on_b)
        self._create(ctx, n_players, rows, C.byref(a), C.byref(b))

    def _schedule(self, out_len, max_spans, table_a, names_a, table_b, names_b):
        """-> the return code"""
        fa = (abi.ScriptSpanParam * len(names_a))(*[table_a.arrays[n] for n in names_a])
        fb = (abi.ScriptSpanParam * len(names_b))(*[table_b.arrays[n] for n in names_b])
        return self.lib.zh_span_merge_schedule(self.handle, out_len, max_spans, C.byref(table_a.tb), fa, C.byref(table_b.tb), fb)

    def schedule(self, out_len, max_spans, table_a, names_a, table_b, names_b):
        """one buffer: enqueued, no sync.  `table_x`: a span table view (.tb, .arrays) such as a bank's script_table(); `names_x`:
        which of its arrays are the source's fields, in the order of fields_x"""
        abi.check(self._schedule(out_len, max_spans, table_a, names_a, table_b, names_b), "zh_span_merge_schedule")


class TwoKeys:
    """keyEvent of examples/example_two.zig (:156-177) for one player, without the queues.  note_key(key, down, rel_freq) is the
    first half (:157-165) -> the (note_id, freq, note_on) to push to source 0, or None; number_key(index, down), index = key -
    SDLK_1 in 0..8, the second (:166-175) -> the (note_id, color, note_on) to push to source 1, or None.  Each source has its own
    key: a press always counts and becomes it, a release counts only for it.  Every push draws a fresh id from its source's
    generator; id 1 of each is the `first` push of :71-81 (first())."""

    def __init__(self, a4=A4):
        self.a4 = np.float32(a4)
        self.key0 = self.key1 = None
        self._next0 = self._next1 = 1

    def _id0(self):
        self._next0 += 1
        return self._next0 - 1

    def _id1(self):
        self._next1 += 1
        return self._next1 - 1

    def first(self):
        """:71-81 -> ((note_id, a4 * 0.5, off), (note_id, 0.5, off)), both at frame 0"""
        return (self._id0(), np.float32(self.a4 * np.float32(0.5)), False), (self._id1(), np.float32(0.5), False)

    def note_key(self, key, down, rel_freq):
        if not (down or self.key0 == key):                             # :158
            return None
        self.key0 = key if down else None                              # :159
        return self._id0(), np.float32(self.a4 * np.float32(rel_freq)), bool(down)   # :160-163

    def number_key(self, index, down):
        if not 0 <= index <= 8:                                        # :166
            raise ValueError("index: 0 to 8 (SDLK_1 to SDLK_9)")
        if not (down or self.key1 == index):                           # :168
            return None
        self.key1 = index if down else None                            # :169
        f = np.float32(index) / np.float32(8)                          # :167
        color = np.float32(0.5) + np.sqrt(f, dtype=np.float32) * np.float32(0.5)   # :171, in f32
        return self._id1(), np.float32(color), bool(down)


class TwoPlayer:
    """N x examples/example_two.zig MainModule.  note_key(player, key, down, rel_freq, frame) and number_key(player, index, down,
    frame) are the two halves of keyEvent :156-177 per player (TwoKeys); paint(frames) is MainModule.paint (:65-154).  The `first`
    pushes of :71-81 -- (a4 * 0.5, off) and (0.5, off) at frame 0 -- are made at construction, before any key, where the reference
    makes them in its first paint: the queues hold them first either way.  Two LiveVoiceBanks of polyphony 1 carry the records
    {freq, note_on, on = 1} and {color, note_on, on = 1}; the banks' note-on byte is the constant `on`, so every push reaches the
    bare Trigger, note-offs included."""

    def __init__(self, ctx, n_players, sample_rate=48000, a4=A4, patch=None, max_impulses=None):
        self.ctx, self.n_players, self.sample_rate = ctx, int(n_players), float(sample_rate)
        self.stage = self.bank0 = self.bank1 = self.voices = None
        self.stage = SpanMerge(ctx, self.n_players, [("freq", "f"), ("note_on_a", "u")], "note_on_a", [("color", "f"), ("note_on_b", "u")], "note_on_b")
        self.keys = [TwoKeys(a4) for _ in range(self.n_players)]
        cap = 33 * self.n_players if max_impulses is None else int(max_impulses)
        self.bank0 = LiveVoiceBank(ctx, self.n_players, 1, FREQ_PARAMS, FREQ_PARAMS.fields["on"][1], cap, rows=SOURCE_SPANS)
        self.bank1 = LiveVoiceBank(ctx, self.n_players, 1, COLOR_PARAMS, COLOR_PARAMS.fields["on"][1], cap, rows=SOURCE_SPANS)
        word = lambda dt, name: dt.fields[name][1] // 4
        self._in0 = self.bank0.script_table(SOURCE_SPANS, {"freq": (word(FREQ_PARAMS, "freq"), "f"), "note_on": (word(FREQ_PARAMS, "note_on"), "u")})
        self._in1 = self.bank1.script_table(SOURCE_SPANS, {"color": (word(COLOR_PARAMS, "color"), "f"), "note_on": (word(COLOR_PARAMS, "note_on"), "u")})
        self._table = self.stage.script_table(MAX_SPANS)
        self.voices = mod.Dual(self.n_players, ctx)
        self._params = mod.Dual.Params(self.sample_rate, patch=patch)        # every field has a span array
        self._frames = 0
        for p in range(self.n_players):                                     # :71-81
            first0, first1 = self.keys[p].first()
            self._push0(p, 0, first0)
            self._push1(p, 0, first1)

    def _push0(self, player, frame, ev):
        rec = np.zeros(1, FREQ_PARAMS)
        rec["freq"], rec["note_on"], rec["on"] = ev[1], int(ev[2]), 1
        self.bank0.push(player, frame, ev[0], rec)

    def _push1(self, player, frame, ev):
        rec = np.zeros(1, COLOR_PARAMS)
        rec["color"], rec["note_on"], rec["on"] = ev[1], int(ev[2]), 1
        self.bank1.push(player, frame, ev[0], rec)

    def note_key(self, player, key, down, rel_freq, frame):
        """-> the (note_id, freq, note_on) pushed, or None where the reference ignores the event"""
        ev = self.keys[player].note_key(key, down, rel_freq)
        if ev is not None:
            self._push0(player, frame, ev)
        return ev

    def number_key(self, player, index, down, frame):
        """-> the (note_id, color, note_on) pushed, or None where the reference ignores the event"""
        ev = self.keys[player].number_key(index, down)
        if ev is not None:
            self._push1(player, frame, ev)
        return ev

    def paint(self, frames):
        """one buffer -> (audio, sync), each [n_players][frames] f32 on the device (views of buffers the next call overwrites): two
        bank schedules, one merge and one zero-first span paint.  All four are enqueued; nothing synchronises."""
        if frames > self._frames:
            self._audio, self._sync = (self.ctx.image(frames, self.n_players) for _ in range(2))
            self._frames = frames
        self.bank0.schedule(frames, SOURCE_SPANS)
        self.bank1.schedule(frames, SOURCE_SPANS)
        self.stage.schedule(frames, MAX_SPANS, self._in0, ("freq", "note_on"), self._in1, ("color", "note_on"))
        audio, sync = self._audio[:frames], self._sync[:frames]
        self.voices.paint_spans(zang.Span(0, frames), [audio, sync], None, self._params, self._table, zero_first=True)
        return audio.t(), sync.t()

    def overflows(self):
        return self.bank0.overflows() + self.bank1.overflows() + self.stage.overflows()

    def close(self):
        for o in (self.voices, self.stage, self.bank0, self.bank1):
            if o is not None:
                o.close()
