"""MousePlayer: N of the reference's mouse example played live (examples/example_mouse.zig MainModule :75-247): a phase-modulation
instrument whose modulator ratio and multiplier are SIGNALS, each painted by its own Portamento from its own impulse stream (the
mouse axes), while the notes come from a third (the keyboard).  Per buffer: each stream's pushed records go through one
LiveVoiceBank launch (the three ImpulseQueue -> Trigger pairs, :151, :174-175, :194; polyphony 1) and ONE zh_pmctl_paint_controlled
with zero-first walks the three tables side by side, the two control signals in registers (:148-211).  Nothing runs on the host per
player; no control image exists."""
import numpy as np
import torch

from . import modules as mod, zang
from .bank import LiveVoiceBank

# the streams' records: Instr.Params (:83) and Porta.Params (:92), and a word that is always set for the bank's dispatcher (every
# push takes slot 0, note-offs included: the bare Triggers of MainModule.paint)
NOTE_PARAMS = np.dtype([("freq", "<f4"), ("note_on", "<u4"), ("on", "<u4")])
CTL_PARAMS = np.dtype([("value", "<f4"), ("note_on", "<u4"), ("on", "<u4")])
STREAM_SPANS = 34                               # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
A4 = 440.0                                      # :22
RATIO_SCALES = (4.0, 880.0)                     # by mode   :161-164
MULTIPLIER_SCALE = 2.0                          # :185


class MouseKeys:
    """keyEvent of examples/example_mouse.zig (:230-246) for one player, without the queues: key(key, down, rel_freq) -> the (note_id,
    freq, note_on) to push to the instrument's stream, or None where the reference ignores the event (a release of a key that is
    not the held one); space() toggles the mode (:231-235).  mode_iq is pushed to and never consumed in the reference: not built."""

    def __init__(self, a4=A4):
        self.a4 = np.float32(a4)
        self.held, self.mode = None, 0
        self._next = 1

    def space(self):
        self.mode = (self.mode + 1) % 2                                # :232
        return self.mode

    def key(self, key, down, rel_freq):
        if not (down or self.held == key):                             # :237
            return None
        self.held = key if down else None                              # :238
        self._next += 1
        return self._next - 1, np.float32(self.a4 * np.float32(rel_freq)), bool(down)   # :239-242


class MousePlayer:
    """N x examples/example_mouse.zig MainModule.  mouse(player, x, y, frame) is mouseEvent :214-228, key(player, key, down,
    rel_freq, frame) the key half of keyEvent :236-244 (MouseKeys), space(player) its first half :231-235; paint(frames) is
    MainModule.paint :138-212.  `mode` is read when a buffer is painted: a toggle holds for the whole of the next paint; it sets
    relative = (mode == 0) and the ratio's scale, 4.0 or 880.0, through per-player device arrays.  Three LiveVoiceBanks of polyphony
    1 carry the records {freq | value, note_on, on = 1}; the banks' note-on byte is the constant `on`, so every push reaches the
    bare Trigger, note-offs included.  exact_temps: keep the image the reference's stale temp lives in (zh_pmctl_*, "ONE
    DIFFERENCE"), so that the output is the reference's bit for bit; without it that temp reads as zero."""

    def __init__(self, ctx, n_players, sample_rate=48000, a4=A4, patch=None, exact_temps=True, max_impulses=None):
        self.ctx, self.n_players, self.sample_rate = ctx, int(n_players), float(sample_rate)
        self.exact_temps = bool(exact_temps)
        self.banks, self.voices = [], None
        self.keys = [MouseKeys(a4) for _ in range(self.n_players)]
        self._ctl_ids = [1] * self.n_players                           # the two control streams draw ids in step (:220-227)
        cap = 33 * self.n_players if max_impulses is None else int(max_impulses)
        word = lambda dt, name: dt.fields[name][1] // 4
        self._tables = []
        for dt, value in ((NOTE_PARAMS, "freq"), (CTL_PARAMS, "value"), (CTL_PARAMS, "value")):
            bank = LiveVoiceBank(ctx, self.n_players, 1, dt, dt.fields["on"][1], cap, rows=STREAM_SPANS)
            self.banks.append(bank)
            self._tables.append(bank.script_table(STREAM_SPANS, {value: (word(dt, value), "f"), "note_on": (word(dt, "note_on"), "u")}))
        self.voices = mod.PMCtl(self.n_players, ctx)
        self._patch = patch
        self._mode = np.zeros(self.n_players, np.uint8)                # what the device arrays hold
        self._relative = torch.ones(self.n_players, dtype=torch.uint8, device=ctx.device)
        self._ratio_scale = torch.full((self.n_players,), RATIO_SCALES[0], dtype=torch.float32, device=ctx.device)
        self._frames = 0
        self._audio = self._stale = None

    def mouse(self, player, x, y, frame):
        """mouseEvent :214-228: x to the ratio's stream, y to the multiplier's, both note-ons with a fresh id"""
        note_id = self._ctl_ids[player]
        self._ctl_ids[player] += 1
        for bank, value in ((self.banks[1], x), (self.banks[2], y)):
            rec = np.zeros(1, CTL_PARAMS)
            rec["value"], rec["note_on"], rec["on"] = np.float32(value), 1, 1
            bank.push(player, frame, note_id, rec)

    def key(self, player, key, down, rel_freq, frame):
        """-> the (note_id, freq, note_on) pushed, or None where the reference ignores the event"""
        ev = self.keys[player].key(key, down, rel_freq)
        if ev is not None:
            rec = np.zeros(1, NOTE_PARAMS)
            rec["freq"], rec["note_on"], rec["on"] = ev[1], int(ev[2]), 1
            self.banks[0].push(player, frame, ev[0], rec)
        return ev

    def space(self, player):
        """-> the player's new mode; it takes effect with the next paint"""
        return self.keys[player].space()

    def _upload_modes(self):
        mode = np.array([k.mode for k in self.keys], np.uint8)
        if not np.array_equal(mode, self._mode):                       # copies enqueued on the paints' stream
            self._mode = mode
            self._relative.copy_(torch.from_numpy((mode == 0).astype(np.uint8)))
            self._ratio_scale.copy_(torch.from_numpy(np.where(mode == 0, np.float32(RATIO_SCALES[0]), np.float32(RATIO_SCALES[1])).astype(np.float32)))

    def paint(self, frames):
        """one buffer -> audio [n_players][frames] f32 on the device (a view of a buffer the next call overwrites): three bank
        schedules and one zero-first controlled paint, all enqueued; nothing synchronises"""
        if frames > self._frames:
            self._audio = self.ctx.image(frames, self.n_players)
            if self.exact_temps:                                       # the carried temp: what it held is kept
                stale = self.ctx.image(frames, self.n_players, fill=0.0)
                if self._stale is not None:
                    stale[:self._frames].copy_(self._stale)
                self._stale = stale
            self._frames = frames
        self._upload_modes()
        for bank in self.banks:
            bank.schedule(frames, STREAM_SPANS)
        audio = self._audio[:frames]
        params = mod.PMCtl.Params(self.sample_rate, relative=self._relative, patch=self._patch)     # freq and note_on: span arrays
        self.voices.paint_controlled(zang.Span(0, frames), [audio], [None, self._stale, None] if self.exact_temps else None, params,
                                     self._tables[0], mod.PMCtl.Control(self._tables[1], self._ratio_scale),
                                     mod.PMCtl.Control(self._tables[2], MULTIPLIER_SCALE), zero_first=True)
        return audio.t()

    def overflows(self):
        return sum(bank.overflows() for bank in self.banks)

    def close(self):
        for o in [self.voices] + self.banks:
            if o is not None:
                o.close()
        self.banks, self.voices = [], None
