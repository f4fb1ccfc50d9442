"""SubsongPlayer: N of the reference's subsong example played live (examples/example_subsong.zig MainModule :147-202): every key
press plays a canned melody, "notes within notes".  Per buffer: the pushed key records go through one LiveVoiceBank launch
(MainModule's ImpulseQueue -> Trigger, :176-185; polyphony 1), one subsong-stage launch turns every outer sub-span into the melody's
notes scaled to the key (SubtrackPlayer.paint :122-144, zh_subsong_schedule) and one SawEnv span paint with zero-first renders them
(InnerInstrument :43-67).  Nothing runs on the host per player."""
import ctypes as C

import numpy as np

from . import abi, modules as mod, zang
from .bank import LiveVoiceBank
from .stage import Stage, StageTable

# the outer record: SubtrackPlayer.Params (:92-96) without the shared sample rate, and which of the kit's melodies the press plays
KEY_PARAMS = np.dtype([("freq", "<f4"), ("note_on", "<u4"), ("melody", "<u4")])
OUTER_SPANS = 34                                # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
MAX_SPANS = 66                                  # rows of the stage's table; one outer sub-span makes at most 33
NO_MELODY = abi.SUBSONG_NO_MELODY
A4 = 440.0
C4 = 0.5946035575013605                         # zang-12tet's c4 relative to a4: 2^(-9/12)
BASE_FREQ = A4 * C4                             # SubtrackPlayer.BaseFrequency (:98)


class MelodyKit:
    """zh_melody_kit_*: K melodies resident on the device, immutable.  `melodies`: a list of melodies, each a list of events
    (t seconds, note_id, freq, note_on) in chronological order."""

    def __init__(self, ctx, melodies):
        self.ctx, self.lib = ctx, ctx.lib
        melodies = [list(m) for m in melodies]
        offsets = np.zeros(len(melodies) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(m) for m in melodies])
        ev = np.zeros(max(int(offsets[-1]), 1), np.dtype(abi.MelodyEvent))
        i = 0
        for m in melodies:
            for t, note_id, freq, note_on in m:
                ev["t"][i], ev["note_id"][i], ev["freq"][i], ev["note_on"][i] = t, note_id, freq, bool(note_on)
                i += 1
        self.handle = C.c_void_p()
        abi.check(self.lib.zh_melody_kit_create(ctx.handle, offsets.ctypes.data, len(melodies), ev.ctypes.data, int(offsets[-1]),
                                                C.byref(self.handle)), "zh_melody_kit_create")
        self.n_melodies = len(melodies)
        ctx._children.add(self)

    def close(self):
        if self.handle:
            self.lib.zh_melody_kit_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


SubsongTable = StageTable


class SubsongStage(Stage):
    """zh_subsong_*: n players' SubtrackPlayer.paint without the instrument.  `kit`: the MelodyKit they play from (it must outlive
    the stage); `base_freq`: the frequency the melodies are written at (:98).  schedule() reads the table of a LiveVoiceBank of
    polyphony 1 whose records are KEY_PARAMS and fills the stage's own table (script_table())."""
    PREFIX = "zh_subsong"
    FIELDS = (("freq", abi.SUBSONG_SPAN_FREQ), ("note_on", abi.SUBSONG_SPAN_NOTE_ON))

    def __init__(self, ctx, n_players, kit, base_freq=BASE_FREQ, rows=None):
        self.kit = kit
        self._create(ctx, n_players, rows, kit.handle, float(base_freq))

    def reset(self):
        abi.check(self.lib.zh_subsong_reset(self.handle), "zh_subsong_reset")

    def _schedule(self, sample_rate, out_len, max_spans, outer):
        """-> the return code; `outer`: a BankScriptTable with the fields freq, note_on and melody"""
        sp = (abi.ScriptSpanParam * abi.SUBSONG_IN_FIELDS)(outer.arrays["freq"], outer.arrays["note_on"], outer.arrays["melody"])
        return self.lib.zh_subsong_schedule(self.handle, float(sample_rate), out_len, max_spans, C.byref(outer.tb), sp)

    def schedule(self, sample_rate, out_len, max_spans, outer):
        """one buffer: enqueued, no sync"""
        abi.check(self._schedule(sample_rate, out_len, max_spans, outer), "zh_subsong_schedule")

    def state(self):
        st = np.zeros(max(self.n_players, 1), np.dtype(abi.SubsongState))
        abi.check(self.lib.zh_subsong_get_state(self.handle, st.ctypes.data), "zh_subsong_get_state")
        return st[:self.n_players]

    def set_state(self, st):
        st = np.ascontiguousarray(st, np.dtype(abi.SubsongState))
        assert st.shape == (self.n_players,)
        abi.check(self.lib.zh_subsong_set_state(self.handle, st.ctypes.data), "zh_subsong_set_state")

    def download(self, max_spans):
        """the stage's table as host arrays (synchronises; for tests and debugging): count [N], start / end / note_on [K][N]
        uint32, freq [K][N] float32, nic [K][N] uint8.  Rows at or above a player's count hold whatever was there."""
        return super().download(max_spans, {"freq": np.float32})


def key_table(bank, max_spans):
    """the view of a KEY_PARAMS bank's table that SubsongStage.schedule takes"""
    word = lambda name: KEY_PARAMS.fields[name][1] // 4
    return bank.script_table(max_spans, {"freq": (word("freq"), "f"), "note_on": (word("note_on"), "u"), "melody": (word("melody"), "u")})


class SubsongKey:
    """keyEvent of examples/example_subsong.zig (:188-201) for one player, without the queue.  event(key, down) -> the
    (note_id, note_on) to push, or None: a press always counts and becomes the key that is down; a release counts only for the
    key that is down.  Every event that counts draws a fresh id (:192).  A LiveVoiceBank routes a note-off by the id of the note
    that is on (PolyphonyDispatcher), so the note-off goes out under THAT id: the stage does not read a note-off's
    note_id_changed, and the next press has a fresh id either way; no bit differs."""

    def __init__(self):
        self.key, self._next_id, self._on_id = None, 1, None

    def event(self, key, down):
        if not (down or self.key == key):                              # :190
            return None
        self.key = key if down else None                               # :191
        note_id = self._next_id                                        # :192
        self._next_id += 1
        if down:
            self._on_id = note_id
        else:
            note_id, self._on_id = self._on_id, None
        return note_id, bool(down)


class SubsongPlayer:
    """N x examples/example_subsong.zig MainModule over a kit of melodies.  key_event(player, key, down, frame, melody=0) is
    keyEvent :188-201 per player (SubsongKey), `key` the frequency the press plays the melody at (the reference's a4 * rel_freq)
    and what identifies the key; paint(frames) is MainModule.paint (:170-186).  `max_spans`: rows of the stage's table per player
    and buffer; a buffer with k key events can make up to (k + 1) * 33 sub-spans, what does not fit is dropped and counted
    (overflows())."""

    def __init__(self, ctx, n_players, kit, sample_rate=48000, base_freq=BASE_FREQ, max_spans=MAX_SPANS, patch=None, max_impulses=None):
        self.ctx, self.n_players, self.sample_rate, self.max_spans = ctx, int(n_players), float(sample_rate), int(max_spans)
        self.stage = self.bank = self.voices = None
        self.stage = SubsongStage(ctx, self.n_players, kit, base_freq, rows=self.max_spans)
        self.keys = [SubsongKey() for _ in range(self.n_players)]
        self.bank = LiveVoiceBank(ctx, self.n_players, 1, KEY_PARAMS, KEY_PARAMS.fields["note_on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=OUTER_SPANS)
        self._outer = key_table(self.bank, OUTER_SPANS)
        self._table = self.stage.script_table(self.max_spans)
        self.voices = mod.SawEnv(self.n_players, ctx)
        self._params = mod.SawEnv.Params(self.sample_rate, patch=patch)      # both fields have a span array
        self._frames = 0

    def key_event(self, player, key, down, frame, melody=0):
        """-> the (note_id, note_on) pushed, or None where the reference ignores the event"""
        ev = self.keys[player].event(float(key), down)
        if ev is not None:
            rec = np.zeros(1, KEY_PARAMS)
            rec["freq"], rec["note_on"], rec["melody"] = key, int(ev[1]), melody
            self.bank.push(player, frame, ev[0], rec)
        return ev

    def paint(self, frames):
        """one buffer -> audio [n_players][frames] f32 on the device (a view of a buffer the next call overwrites): one bank
        schedule, one stage schedule and one span paint.  All three are enqueued; nothing synchronises."""
        if frames > self._frames:
            self._audio = self.ctx.image(frames, self.n_players)
            self._frames = frames
        self.bank.schedule(frames, OUTER_SPANS)
        self.stage.schedule(self.sample_rate, frames, self.max_spans, self._outer)
        audio = self._audio[:frames]
        self.voices.paint_spans(zang.Span(0, frames), [audio], None, self._params, self._table, zero_first=True)
        return audio.t()

    def overflows(self):
        return self.bank.overflows() + self.stage.overflows()

    def close(self):
        for o in (self.voices, self.stage, self.bank):
            if o is not None:
                o.close()
