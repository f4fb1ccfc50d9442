"""DetunedPlayer: N of the reference's detuned examples (examples/example_detuned.zig MainModule, :171-266) played live.  Per
buffer: the pushed impulses go through one LiveVoiceBank launch (ImpulseQueue -> Trigger; polyphony 1, as the example has one
OuterInstrument), one zh_detuned_paint_spans renders every player's sub-spans into a bus image with each impulse's freq,
note_on and mode (:213-222), the bus goes straight to both outputs unless the echo bit is set (:225-230), and one StereoEchoes
launch (voice = player) runs on EVERY buffer (:232-242): with a zero input the delays keep ringing."""
import numpy as np

from . import modules as mod, zang
from .bank import LiveVoiceBank

# the note record: OuterInstrument.Params (:106-111) without the shared sample rate
NOTE_PARAMS = np.dtype([("freq", "<f4"), ("note_on", "<u4"), ("mode", "<u4")])
MAX_SPANS = 34                                  # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1


class DetunedPlayer:
    def __init__(self, ctx, n_players, sample_rate=48000, first_seed=0, main_delay=15000, max_impulses=None, patch=None):
        """`first_seed`: player j's noise is seeded like the (first_seed + j)-th Noise.init().  `max_impulses`: the most pushes
        one buffer may carry over all players (default 33 per player: one more than their queues accept).  `mode` (0-3, shared
        by all players): bit 0 = narrow warble, stored in every pushed impulse, so that a change reaches the instrument with
        the next key (:257-259); bit 1 = echo, read by paint().  Push a note-off for the held note only, as the reference's
        keyEvent does (:251-252): the bank routes a note-off by its note id (PolyphonyDispatcher), the example's bare Trigger
        does not look at it."""
        self.ctx, self.n_players, self.sample_rate = ctx, int(n_players), float(sample_rate)
        self.mode = 0
        self.bank = LiveVoiceBank(ctx, self.n_players, 1, NOTE_PARAMS, NOTE_PARAMS.fields["note_on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=MAX_SPANS)
        word = lambda name: NOTE_PARAMS.fields[name][1] // 4
        self._table = self.bank.script_table(MAX_SPANS, {"freq": (word("freq"), "f"), "note_on": (word("note_on"), "u"), "mode": (word("mode"), "u")})
        self.voices = mod.Detuned(self.n_players, ctx, first_seed)
        self.echoes = mod.StereoEchoes(self.n_players, main_delay, ctx)
        self._params = mod.Detuned.Params(self.sample_rate, patch=patch)      # every field has a span array
        self._frames = 0

    def push(self, player, frame, note_id, freq, note_on):
        """keyEvent's iq.push (:253-260): scalars, or equal-length arrays in push order"""
        freq = np.atleast_1d(np.asarray(freq, np.float32))
        rec = np.zeros(len(freq), NOTE_PARAMS)
        rec["freq"] = freq
        rec["note_on"] = np.asarray(note_on, bool)
        rec["mode"] = self.mode
        self.bank.push(player, frame, note_id, rec)

    def _reserve(self, frames):
        if frames > self._frames:
            self._bus, self._left, self._right = (self.ctx.image(frames, self.n_players) for _ in range(3))
            self._frames = frames

    def paint(self, frames):
        """one buffer -> (left, right), each [n_players][frames] f32 on the device (views of buffers the next call overwrites).
        Every step is enqueued; nothing synchronises."""
        self._reserve(frames)
        span = zang.Span(0, frames)
        self.bank.schedule(frames, MAX_SPANS)
        bus, left, right = self._bus[:frames], self._left[:frames], self._right[:frames]
        self.voices.paint_spans(span, [bus], None, self._params, self._table, zero_first=True)     # :211-223
        zang.zero(span, left, ctx=self.ctx); zang.zero(span, right, ctx=self.ctx)
        if (self.mode & 2) == 0:                                                                    # :225-230
            zang.addInto(span, left, bus, ctx=self.ctx); zang.addInto(span, right, bus, ctx=self.ctx)
            zang.zero(span, bus, ctx=self.ctx)
        self.echoes.paint(span, [left, right], None, False, self.echoes.Params(bus, 0.6, 0.1))     # :232-242
        return left.t(), right.t()

    def overflows(self):
        return self.bank.overflows()

    def close(self):
        for o in (self.voices, self.echoes, self.bank):
            if o is not None:
                o.close()
