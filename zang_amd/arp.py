"""ArpPlayer: N of the reference's arpeggiator example played live (examples/example_arpeggiator.zig MainModule :120-168).  Per
buffer: the pushed held-key records go through one LiveVoiceBank launch (MainModule's ImpulseQueue -> Trigger, :153-156; polyphony
1), one arpeggiator-stage launch turns every outer sub-span into the clocked note-ons and note-offs of Arpeggiator.paint (:49-107,
zh_arp_schedule) and one HardSquare span paint with zero-first renders them into the audio image and the frequency image (the
oscilloscope sync, :106-116).  Nothing runs on the host per player."""
import ctypes as C

import numpy as np

from . import abi, modules as mod, zang
from .bank import LiveVoiceBank
from .stage import Stage, StageTable

# the outer record: Arpeggiator.Params (:26-29) without the shared sample rate -- note_held as a 64-bit mask in two words, and a
# byte that is always set for the bank's dispatcher (every push takes slot 0: the bare Trigger of MainModule.paint)
HELD_PARAMS = np.dtype([("held_lo", "<u4"), ("held_hi", "<u4"), ("on", "<u4")])
MAX_KEYS = 64
OUTER_SPANS = 34                                # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
MAX_SPANS = 64                                  # rows of the stage's table; a call of Arpeggiator.paint makes at most 33


class ArpKeys:
    """keyEvent of examples/example_arpeggiator.zig (:159-167) for one player, without the queue: note_held[key_index] = down on a
    64-bit mask.  key(key_index, down) -> the (note_id, mask) to push: EVERY event is pushed, with a fresh id and the whole mask."""

    def __init__(self, n_keys):
        if not 0 < n_keys <= MAX_KEYS:
            raise ValueError(f"n_keys: 1 to {MAX_KEYS}")
        self.n_keys, self.held, self._next_id = int(n_keys), 0, 1

    def key(self, key_index, down):
        if not 0 <= key_index < self.n_keys:
            raise ValueError("key_index outside the key table")
        flag = 1 << key_index
        self.held = (self.held | flag) if down else (self.held & ~flag)       # :162
        note_id = self._next_id                                              # :163
        self._next_id += 1
        return note_id, self.held


ArpTable = StageTable


class ArpStage(Stage):
    """zh_arp_*: n players' Arpeggiator.paint without the instrument.  `key_freqs`: 1 to 64 key frequencies (the reference's are
    a4 * key_bindings[i].rel_freq), copied to the device.  schedule() reads the table of a LiveVoiceBank of polyphony 1 whose
    records are HELD_PARAMS and fills the stage's own table (script_table())."""
    PREFIX = "zh_arp"
    FIELDS = (("freq", abi.ARP_SPAN_FREQ), ("note_on", abi.ARP_SPAN_NOTE_ON))

    def __init__(self, ctx, n_players, key_freqs, rows=None):
        self.key_freqs = np.ascontiguousarray(np.asarray(key_freqs, np.float32).reshape(-1))
        self._create(ctx, n_players, rows, self.key_freqs.ctypes.data, len(self.key_freqs))

    def reset(self):
        abi.check(self.lib.zh_arp_reset(self.handle), "zh_arp_reset")

    def _schedule(self, sample_rate, out_len, max_spans, outer):
        """-> the return code; `outer`: a BankScriptTable with the fields held_lo and held_hi"""
        held = (abi.ScriptSpanParam * 2)(outer.arrays["held_lo"], outer.arrays["held_hi"])
        return self.lib.zh_arp_schedule(self.handle, float(sample_rate), out_len, max_spans, C.byref(outer.tb), held)

    def schedule(self, sample_rate, out_len, max_spans, outer):
        """one buffer: enqueued, no sync"""
        abi.check(self._schedule(sample_rate, out_len, max_spans, outer), "zh_arp_schedule")

    def state(self):
        st = np.zeros(max(self.n_players, 1), np.dtype(abi.ArpState))
        abi.check(self.lib.zh_arp_get_state(self.handle, st.ctypes.data), "zh_arp_get_state")
        return st[:self.n_players]

    def set_state(self, st):
        st = np.ascontiguousarray(st, np.dtype(abi.ArpState))
        assert st.shape == (self.n_players,)
        abi.check(self.lib.zh_arp_set_state(self.handle, st.ctypes.data), "zh_arp_set_state")

    def download(self, max_spans):
        """the stage's table as host arrays (synchronises; for tests and debugging): count [N], start / end / note_on [K][N]
        uint32, freq [K][N] float32, nic [K][N] uint8.  Rows at or above a player's count hold whatever was there."""
        return super().download(max_spans, {"freq": np.float32})


def held_table(bank, max_spans):
    """the view of a HELD_PARAMS bank's table that ArpStage.schedule takes"""
    word = lambda name: HELD_PARAMS.fields[name][1] // 4
    return bank.script_table(max_spans, {"held_lo": (word("held_lo"), "u"), "held_hi": (word("held_hi"), "u")})


class ArpPlayer:
    """N x examples/example_arpeggiator.zig MainModule.  key(player, key_index, down, frame) is keyEvent :159-167 per player
    (ArpKeys); paint(frames) its paint (:147-157).  `max_spans`: rows of the stage's table per player and buffer; a buffer with k
    key events can make up to (k + 1) * 33 sub-spans, what does not fit is dropped and counted (overflows())."""

    def __init__(self, ctx, n_players, key_freqs, sample_rate=48000, max_spans=MAX_SPANS, max_impulses=None):
        self.ctx, self.n_players, self.sample_rate, self.max_spans = ctx, int(n_players), float(sample_rate), int(max_spans)
        self.stage = self.bank = self.voices = None
        self.stage = ArpStage(ctx, self.n_players, key_freqs, rows=self.max_spans)
        self.keys = [ArpKeys(len(self.stage.key_freqs)) for _ in range(self.n_players)]
        self.bank = LiveVoiceBank(ctx, self.n_players, 1, HELD_PARAMS, HELD_PARAMS.fields["on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=OUTER_SPANS)
        self._outer = held_table(self.bank, OUTER_SPANS)
        self._table = self.stage.script_table(self.max_spans)
        self.voices = mod.HardSquare(self.n_players, ctx)
        self._params = mod.HardSquare.Params(self.sample_rate)                # both fields have a span array
        self._frames = 0

    def key(self, player, key_index, down, frame):
        """-> the (note_id, mask) pushed"""
        note_id, held = self.keys[player].key(key_index, down)
        rec = np.zeros(1, HELD_PARAMS)
        rec["held_lo"], rec["held_hi"], rec["on"] = held & 0xffffffff, held >> 32, 1
        self.bank.push(player, frame, note_id, rec)
        return note_id, held

    def paint(self, frames):
        """one buffer -> (audio, sync), each [n_players][frames] f32 on the device (views of buffers the next call overwrites): one
        bank schedule, one arp schedule and one span paint.  All three are enqueued; nothing synchronises."""
        if frames > self._frames:
            self._audio, self._sync = (self.ctx.image(frames, self.n_players) for _ in range(2))
            self._frames = frames
        self.bank.schedule(frames, OUTER_SPANS)
        self.stage.schedule(self.sample_rate, frames, self.max_spans, self._outer)
        audio, sync = self._audio[:frames], self._sync[:frames]
        self.voices.paint_spans(zang.Span(0, frames), [audio, sync], None, self._params, self._table, zero_first=True)
        return audio.t(), sync.t()

    def overflows(self):
        return self.bank.overflows() + self.stage.overflows()

    def close(self):
        for o in (self.voices, self.stage, self.bank):
            if o is not None:
                o.close()
