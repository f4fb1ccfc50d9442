"""VibratoPlayer and PortaPlayer: N of the reference's monophonic lead examples played live (examples/example_vibrato.zig MainModule
:71-126, examples/example_portamento.zig MainModule :89-176).  Per buffer: the pushed impulses go through one LiveVoiceBank launch
(ImpulseQueue -> Trigger; polyphony 1, as each example has one Instrument) and one span paint with zero-first renders every
player's sub-spans into the audio image and the frequency image (the oscilloscope sync) with each impulse's freq and note_on."""
import numpy as np

from . import modules as mod, zang
from .bank import LiveVoiceBank

# the note record: Instrument.Params (portamento :23-27, vibrato :20-24) without the shared sample rate
NOTE_PARAMS = np.dtype([("freq", "<f4"), ("note_on", "<u4")])
MAX_SPANS = 34                                  # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
MAX_KEYS = 64                                   # keys_held is a u64 (portamento :97)


class _LeadPlayer:
    _voice = None                               # mod.Vibrato / mod.Porta

    def __init__(self, ctx, n_players, sample_rate=48000, patch=None, max_impulses=None):
        """`max_impulses`: the most pushes one buffer may carry over all players (default 33 per player: one more than their
        queues accept).  Push a note-off with the id of the note that is on: the bank routes a note-off by its note id
        (PolyphonyDispatcher), the examples' bare Trigger does not look at it."""
        self.ctx, self.n_players, self.sample_rate = ctx, int(n_players), float(sample_rate)
        self.bank = LiveVoiceBank(ctx, self.n_players, 1, NOTE_PARAMS, NOTE_PARAMS.fields["note_on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=MAX_SPANS)
        word = lambda name: NOTE_PARAMS.fields[name][1] // 4
        self._table = self.bank.script_table(MAX_SPANS, {"freq": (word("freq"), "f"), "note_on": (word("note_on"), "u")})
        self.voices = self._voice(self.n_players, ctx)
        self._params = self._voice.Params(self.sample_rate, patch=patch)      # both fields have a span array
        self._frames = 0

    def push(self, player, frame, note_id, freq, note_on):
        """keyEvent's iq.push: scalars, or equal-length arrays in push order"""
        freq = np.atleast_1d(np.asarray(freq, np.float32))
        rec = np.zeros(len(freq), NOTE_PARAMS)
        rec["freq"] = freq
        rec["note_on"] = np.asarray(note_on, bool)
        self.bank.push(player, frame, note_id, rec)

    def paint(self, frames):
        """one buffer -> (audio, sync), each [n_players][frames] f32 on the device (views of buffers the next call overwrites): one
        bank schedule and one span paint.  Both are enqueued; nothing synchronises."""
        if frames > self._frames:
            self._audio, self._sync = (self.ctx.image(frames, self.n_players) for _ in range(2))
            self._frames = frames
        self.bank.schedule(frames, MAX_SPANS)
        audio, sync = self._audio[:frames], self._sync[:frames]
        self.voices.paint_spans(zang.Span(0, frames), [audio, sync], None, self._params, self._table, zero_first=True)
        return audio.t(), sync.t()

    def overflows(self):
        return self.bank.overflows()

    def close(self):
        for o in (self.voices, self.bank):
            if o is not None:
                o.close()


class VibratoPlayer(_LeadPlayer):
    """N x examples/example_vibrato.zig MainModule: push(player, frame, note_id, freq, note_on) is its keyEvent's iq0.push
    (:117-121), paint(frames) its paint (:95-111)"""
    _voice = mod.Vibrato


class PortaKeys:
    """keyEvent of examples/example_portamento.zig (:135-173) for one player, without the queue: the analog-mono rule on a 64-bit
    keys_held.  key(key_index, down) -> the (note_id, freq, note_on) to push, or None.
      a key down pushes only if its flag exceeds keys_held before the press (:148): not a lower key under a higher one, not a repeat;
      a key up pushes a note-off if nothing is held (:158-163), else a note-on at the highest held key's frequency (:164-171).
    Every push draws a fresh id from the player's IdGenerator (:99), as the reference's does.  A LiveVoiceBank routes a note-off by
    the id of the note that is on (PolyphonyDispatcher), so a note-off goes out under THAT id: the voice does not read a note-off's
    note_id_changed, no bit differs.  Not pushed, unlike the reference: a second note-off in a row (a key that was not down
    released while nothing is held) -- the bank has no note to route it to."""

    def __init__(self, key_freqs):
        self.key_freqs = np.asarray(key_freqs, np.float32).reshape(-1)
        if not 0 < len(self.key_freqs) <= MAX_KEYS:
            raise ValueError(f"key_freqs: 1 to {MAX_KEYS} frequencies")
        self.keys_held = 0
        self._next_id = 1
        self._on_id = None                              # the id of the note that is on, None after a note-off

    def key(self, key_index, down):
        if not 0 <= key_index < len(self.key_freqs):
            raise ValueError("key_index outside key_freqs")
        flag = 1 << key_index
        prev = self.keys_held
        if down:
            self.keys_held = prev | flag                              # :146
            if flag <= prev:                                          # :148
                return None
            freq, note_on = self.key_freqs[key_index], True
        else:
            self.keys_held = prev & ~flag                             # :156
            if self.keys_held == 0:                                   # :158-163
                freq, note_on = self.key_freqs[key_index], False
            else:                                                     # :164-171: the highest key still held
                freq, note_on = self.key_freqs[self.keys_held.bit_length() - 1], True
        note_id = self._next_id
        self._next_id += 1
        if note_on:
            self._on_id = note_id
        else:
            if self._on_id is None:
                return None
            note_id, self._on_id = self._on_id, None
        return note_id, float(freq), note_on


class PortaPlayer(_LeadPlayer):
    """N x examples/example_portamento.zig MainModule.  `key_freqs`: the caller's table of at most 64 key frequencies, ascending
    by key index (the reference's is a4 * key_bindings[i].rel_freq).  key(player, key_index, down, frame) is keyEvent :135-173
    per player (PortaKeys): the highest held key sounds, and a note-off is sent only when every key is up."""
    _voice = mod.Porta

    def __init__(self, ctx, n_players, key_freqs, sample_rate=48000, patch=None, max_impulses=None):
        self.keys = [PortaKeys(key_freqs) for _ in range(int(n_players))]
        super().__init__(ctx, n_players, sample_rate, patch, max_impulses)

    def key(self, player, key_index, down, frame):
        """-> the (note_id, freq, note_on) pushed, or None"""
        ev = self.keys[player].key(key_index, down)
        if ev is not None:
            self.push(player, frame, *ev)
        return ev
