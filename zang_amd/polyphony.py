"""PolyphonyPlayer: N of the reference's key-per-voice polyphony example played live (examples/example_polyphony.zig MainModule
:99-179).  Per buffer: the pushed held-key records go through one LiveVoiceBank launch (MainModule's ImpulseQueue -> Trigger,
:137-145; polyphony 1), one key fan-out launch turns every outer sub-span into each key's own sub-spans (Polyphony.paint :61-92,
zh_keyfan_schedule), one NiceInstrument span paint with zero-first renders all N x n_keys always-running voices, and one decimated
group mix adds each player's voices in key order and takes the bus through the player's Decimator or past it (:147-163,
zh_decimator_paint_groups).  Nothing runs on the host per voice."""
import ctypes as C

import numpy as np

from . import abi, modules as mod, zang
from .arp import HELD_PARAMS, OUTER_SPANS, ArpKeys, held_table
from .bank import LiveVoiceBank
from .stage import Stage

MAX_SPANS = 34                                  # an outer sub-span makes at most one row a voice: what OUTER_SPANS is to the bank
DEC_RATES = (0.0, 6000.0, 5000.0, 4000.0, 3000.0, 2000.0, 1000.0)   # :151-158 by dec_mode; mode 0 is the bypass (:161-163)


class KeyFanSpanTable:
    """What NiceInstrument / PMOscInstrument.paint_spans take (zh_span_table): a view of the stage's table."""

    def __init__(self, stage, max_spans):
        self.stage, self.max_spans = stage, max_spans
        self.c = abi.SpanTable()
        stage._call("span_table", max_spans, C.byref(self.c))


class KeyFanStage(Stage):
    """zh_keyfan_*: n players' Polyphony.paint without the instruments, one table column per voice = player * n_keys + key.
    `key_freqs`: 1 to 64 key frequencies (the reference's are a4 * key_bindings[i].rel_freq), copied to the device.  schedule() reads
    the table of a LiveVoiceBank of polyphony 1 whose records are arp.HELD_PARAMS and fills the stage's own table (span_table() for
    NiceInstrument and PMOscInstrument, script_table() for the other span paints)."""
    PREFIX = "zh_keyfan"
    FIELDS = (("freq", abi.KEYFAN_SPAN_FREQ), ("note_on", abi.KEYFAN_SPAN_NOTE_ON))

    def __init__(self, ctx, n_players, key_freqs, rows=None):
        self.key_freqs = np.ascontiguousarray(np.asarray(key_freqs, np.float32).reshape(-1))
        self.n_keys, self.n_outer = len(self.key_freqs), int(n_players)
        self._create(ctx, n_players, rows, self.key_freqs.ctypes.data, self.n_keys)
        self.n_players = self.n_outer * self.n_keys                            # the table's columns (Stage: StageTable, download)

    def reset(self):
        abi.check(self.lib.zh_keyfan_reset(self.handle), "zh_keyfan_reset")

    def _schedule(self, out_len, max_spans, outer):
        """-> the return code; `outer`: a BankScriptTable with the fields held_lo and held_hi"""
        held = (abi.ScriptSpanParam * 2)(outer.arrays["held_lo"], outer.arrays["held_hi"])
        return self.lib.zh_keyfan_schedule(self.handle, out_len, max_spans, C.byref(outer.tb), held)

    def schedule(self, out_len, max_spans, outer):
        """one buffer: enqueued, no sync"""
        abi.check(self._schedule(out_len, max_spans, outer), "zh_keyfan_schedule")

    def span_table(self, max_spans):
        return KeyFanSpanTable(self, max_spans)

    def state(self):
        st = np.zeros(max(self.n_players, 1), np.dtype(abi.KeyFanState))
        abi.check(self.lib.zh_keyfan_get_state(self.handle, st.ctypes.data), "zh_keyfan_get_state")
        return st[:self.n_players]

    def set_state(self, st):
        st = np.ascontiguousarray(st, np.dtype(abi.KeyFanState))
        assert st.shape == (self.n_players,)
        abi.check(self.lib.zh_keyfan_set_state(self.handle, st.ctypes.data), "zh_keyfan_set_state")

    def download(self, max_spans):
        """the stage's table as host arrays (synchronises; for tests and debugging): count [V], start / end / note_on [K][V]
        uint32, freq [K][V] float32, nic and note_on8 (the byte plane of span_table()) [K][V] uint8, V = players x keys.  Rows at
        or above a voice's count hold whatever was there."""
        out = super().download(max_spans, {"freq": np.float32})
        on8 = np.zeros((max_spans, self.n_players), np.uint8)
        if on8.size:
            abi.check(self.lib.zh_download(self.ctx.handle, on8.ctypes.data, self.span_table(max_spans).c.note_on, on8.nbytes), "zh_download")
        out["note_on8"] = on8
        return out


class PolyphonyPlayer:
    """N x examples/example_polyphony.zig MainModule.  key(player, key_index, down, frame) is keyEvent :171-176 per player
    (arp.ArpKeys); space(player) the space bar (:167-169); paint(frames) its paint (:129-164).  `max_spans`: rows of the stage's
    table per voice and buffer; 34 hold whatever the outer queue of 32 impulses makes."""

    def __init__(self, ctx, n_players, key_freqs, color=0.3, sample_rate=48000, max_spans=MAX_SPANS, max_impulses=None):
        self.ctx, self.n_players, self.sample_rate, self.max_spans = ctx, int(n_players), float(sample_rate), int(max_spans)
        self.stage = self.bank = self.voices = self.dec = None
        self.stage = KeyFanStage(ctx, self.n_players, key_freqs, rows=self.max_spans)
        self.n_keys = self.stage.n_keys
        self.keys = [ArpKeys(self.n_keys) for _ in range(self.n_players)]
        self.bank = LiveVoiceBank(ctx, self.n_players, 1, HELD_PARAMS, HELD_PARAMS.fields["on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=OUTER_SPANS)
        self._outer = held_table(self.bank, OUTER_SPANS)
        self._table = self.stage.span_table(self.max_spans)
        self.voices = mod.NiceInstrument(self.n_players * self.n_keys, color, ctx)     # Instrument.init(0.3), :54
        self.dec = mod.Decimator(self.n_players, ctx)                                   # :124
        self.dec_mode = [0] * self.n_players                                            # :125
        self._modes = None                                                              # the device copy; None: to be uploaded
        self._frames = 0

    def key(self, player, key_index, down, frame):
        """-> the (note_id, mask) pushed"""
        note_id, held = self.keys[player].key(key_index, down)
        rec = np.zeros(1, HELD_PARAMS)
        rec["held_lo"], rec["held_hi"], rec["on"] = held & 0xffffffff, held >> 32, 1
        self.bank.push(player, frame, note_id, rec)
        return note_id, held

    def space(self, player):
        """-> the player's new dec_mode"""
        self.dec_mode[player] = (self.dec_mode[player] + 1) % len(DEC_RATES)           # :168
        self._modes = None
        return self.dec_mode[player]

    def paint(self, frames):
        """one buffer -> audio [n_players][frames] f32 on the device (a view of a buffer the next call overwrites): one bank
        schedule, one fan-out schedule, one span paint over all the voices and one decimated group mix.  All four are enqueued;
        nothing synchronises.  (After a space() the players' modes are copied to the device first.)"""
        if frames > self._frames:
            self._image = self.ctx.image(frames, self.n_players * self.n_keys)
            self._audio = self.ctx.image(self.n_players, frames, pad=0)
            self._frames = frames
        if self._modes is None:
            self._modes = self.dec.group_modes([DEC_RATES[m] for m in self.dec_mode], [m == 0 for m in self.dec_mode])
        self.bank.schedule(frames, OUTER_SPANS)
        self.enqueue(frames)
        return self._audio[:, :frames]

    def enqueue(self, frames):
        """paint()'s three launches behind the bank's (which copies the pushed records from the host): what a graph can hold"""
        span, image = zang.Span(0, frames), self._image[:frames]
        self.stage.schedule(frames, self.max_spans, self._outer)
        self.voices.paint_spans(span, [image], None, self.sample_rate, self._table, zero_first=True)
        self.dec.paint_groups(span, self._audio, image, self.n_keys, self.sample_rate, self._modes, zero_first=True)

    def overflows(self):
        return self.bank.overflows() + self.stage.overflows()

    def close(self):
        for o in (self.dec, self.voices, self.stage, self.bank):
            if o is not None:
                o.close()
