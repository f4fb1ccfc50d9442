"""FMSynth: N of the reference's FM synthesizers (examples/example_fmsynth.zig MainModule, :358-520) played live, with no host
work per voice.  Per buffer: the pushed key events go through one LiveVoiceBank launch (ImpulseQueue -> PolyphonyDispatcher(8) ->
Triggers, :453-459), two SineOsc paints fill the tremolo and vibrato LFO images (3.7 Hz and 6.4 Hz, one column per synth,
:437-450), one fused FM paint renders every voice's sub-spans (:460-495), and the grouped mixdown adds each synth's voices in the
reference's order.

That order: the reference adds every voice into ONE buffer, (acc + m_v) + c_v with the modulator's part m_v present in algorithm 0
only (:302, :335).  When any patch has algorithm 0 the voices are painted with ZH_FM_SPLIT_OPERATORS into two columns each and the
mixdown runs over groups of 2 * polyphony columns; otherwise over the plain image in groups of `polyphony`.  Either way the mix
rows have the reference's bits."""
import numpy as np
import torch

from . import abi, modules as mod, zang
from .bank import LiveVoiceBank

NOTE_PARAMS = np.dtype([("freq", "<f4"), ("note_on", "u1"), ("pad", "u1", 3)])       # NoteParams :365-368
TREMOLO_HZ, VIBRATO_HZ = 3.7, 6.4                                                    # :437-450
MAX_SPANS = 34                                  # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1


class FMSynth:
    def __init__(self, ctx, n_synths, patches=None, polyphony=8, sample_rate=48000, max_impulses=None):
        """`patches`: None (the default patch, :376-397), one list of 22 values, or one per synth.  `max_impulses`: the most
        pushes one buffer may carry over all synths (default 32 per synth: what their queues accept)."""
        self.ctx, self.n_synths, self.polyphony, self.sample_rate = ctx, int(n_synths), int(polyphony), float(sample_rate)
        self.n_voices = self.n_synths * self.polyphony
        self.bank = LiveVoiceBank(ctx, self.n_synths, self.polyphony, NOTE_PARAMS, NOTE_PARAMS.fields["note_on"][1],
                                  32 * self.n_synths if max_impulses is None else int(max_impulses), rows=MAX_SPANS)
        self._table = self.bank.span_table(MAX_SPANS, NOTE_PARAMS.fields["freq"][1] // 4)
        self.tremolo_lfo, self.vibrato_lfo = mod.SineOsc(self.n_synths, ctx), mod.SineOsc(self.n_synths, ctx)
        self.voices = mod.FMInstrument(self.n_voices, ctx, group=self.polyphony)
        self.split = False
        self._frames = 0
        if patches is not None:
            self.set_patches(patches)

    def set_patches(self, patches):
        patches = np.ascontiguousarray(patches, dtype=np.uint32)
        if patches.ndim == 1:
            patches = patches[None, :]
        self.voices.set_patches(patches)
        self.split = bool((patches[:, abi.FM_ALGORITHM] == 0).any())
        self._frames = 0                                             # the voice image's width depends on it

    def push(self, synth, frame, note_id, freq, note_on):
        """keyEvent's iq.push (:499-519): scalars, or equal-length arrays in push order"""
        freq, on = np.atleast_1d(np.asarray(freq, np.float32)), np.atleast_1d(np.asarray(note_on)).astype(np.uint8)
        rec = np.zeros(len(freq), NOTE_PARAMS)
        rec["freq"], rec["note_on"] = freq, on
        self.bank.push(synth, frame, note_id, rec)

    def _reserve(self, frames):
        if frames > self._frames:
            cols = self.n_voices * (2 if self.split else 1)
            self._image = self.ctx.image(frames, cols)
            self._lfo = [self.ctx.image(frames, self.n_synths) for _ in range(2)]
            self._mix = torch.zeros((self.n_synths, frames), dtype=torch.float32, device=self.ctx.device)
            self._pcm = torch.zeros((self.n_synths, frames * 2), dtype=torch.uint8, device=self.ctx.device)
            self._frames = frames

    def _paint_voices(self, frames):
        """MainModule.paint up to the voices' image; every step is enqueued, nothing synchronises"""
        self._reserve(frames)
        span = zang.Span(0, frames)
        self.bank.schedule(frames, MAX_SPANS)
        trem, vib = self._lfo[0][:frames], self._lfo[1][:frames]
        for lfo, img, hz in ((self.tremolo_lfo, trem, TREMOLO_HZ), (self.vibrato_lfo, vib, VIBRATO_HZ)):
            lfo.paint(span, [img], [], False, lfo.Params(self.sample_rate, zang.constant(hz), zang.constant(0.0)), zero_first=True)
        img = self._image[:frames]
        self.voices.paint_spans(span, [img], None, self.sample_rate, trem, vib, self._table, zero_first=True, split=self.split)
        return span, img, self.polyphony * (2 if self.split else 1)

    def paint(self, frames):
        """one buffer -> the [n_synths][frames] f32 mix rows, on the device (a view of a buffer the next call overwrites)"""
        span, img, group = self._paint_voices(frames)
        zang.mixdownGroups(span, self._mix, img, group, zero_first=True, ctx=self.ctx)
        return self._mix[:, :frames]

    def paint_pcm(self, frames, vol=0.25):
        """one buffer -> [n_synths][frames * 2] bytes of s16 mono PCM on the device (zang.mixDown of the mix rows)"""
        span, img, group = self._paint_voices(frames)
        zang.mixdownGroupsPcm(span, self._pcm, img, group, zang.AudioFormat.signed16_lsb, 1, 0, vol, ctx=self.ctx)
        return self._pcm[:, :frames * 2]

    def overflows(self):
        return self.bank.overflows()

    def close(self):
        for o in (self.voices, self.tremolo_lfo, self.vibrato_lfo, self.bank):
            o.close()
