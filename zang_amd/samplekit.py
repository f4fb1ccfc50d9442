"""Sample kits: K samples resident on the device (zh_sample_kit), and SamplePlayer -- N of the reference's sampler
examples (examples/example_sampler.zig MainModule, :54-119) played live.  In the reference the sample is a field of the Sampler's
Params (src/modules/Sampler.zig:62-67), so every pushed note names its own (:86-91, :123-138); here a note names an entry of a
kit.  Per buffer: the pushed notes go through one LiveVoiceBank launch (ImpulseQueue -> PolyphonyDispatcher -> Triggers), one
Sampler paint over the bank's tables renders every voice's sub-spans with each note's sample, channel, rate and loop flag
(zh_sampler_paint_kit_spans, :96-105), the grouped mixdown adds each player's voices in voice order, and the example's gain
(:106) and optional overdrive (:108-115) run on the mix rows."""
import ctypes as C
import wave

import numpy as np
import torch

from . import abi, modules as mod, zang
from .bank import LiveVoiceBank

# the note record: Sampler.Params (:62-67) with the sample as an index into the kit, and the note_on the dispatcher reads
NOTE_PARAMS = np.dtype([("sample_rate", "<f4"), ("sample", "<u4"), ("channel", "<u4"), ("loop", "<u4"), ("note_on", "<u4")])
MAX_SPANS = 34                                  # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
GAIN = 2.5                                      # :106
OVERDRIVE = (0.9, 0.5, 0.0)                     # ingain, outgain, offset (:108-115)


def read_wav(path):
    """-> (num_channels, sample_rate, format, bytes) of a PCM .wav file of 1 to 4 bytes per value (the standard library's
    `wave`; examples/example_sampler.zig:15-44 reads its drum loop the same way).  Touches no device."""
    with wave.open(path, "rb") as w:
        width = w.getsampwidth()
        if not 1 <= width <= 4:
            raise ValueError("%s: %d bytes per value" % (path, width))
        return w.getnchannels(), w.getframerate(), width - 1, w.readframes(w.getnframes())


class SampleKit:
    """`samples`: a list of (num_channels, sample_rate, format, data) -- what read_wav returns -- with data as bytes or a uint8
    numpy array on the HOST; the kit copies them to the device once."""

    def __init__(self, ctx, samples):
        self.ctx, self.lib = ctx, ctx.lib
        keep = [np.ascontiguousarray(np.frombuffer(d, np.uint8) if isinstance(d, (bytes, bytearray, memoryview)) else d, np.uint8)
                for _, _, _, d in samples]
        arr = (abi.Sample * max(len(samples), 1))()
        for i, ((nch, rate, fmt, _), d) in enumerate(zip(samples, keep)):
            arr[i] = abi.Sample(int(nch), int(rate), int(fmt), 0, d.ctypes.data if d.size else None, d.size)
        self.handle = C.c_void_p()
        abi.check(self.lib.zh_sample_kit_create(ctx.handle, arr, len(samples), C.byref(self.handle)), "zh_sample_kit_create")
        self.count = len(samples)
        ctx._children.add(self)

    def sample(self, i):
        """entry i as the abi.Sample zh_sampler_paint / zh_sampler_paint_spans take: `data` is its DEVICE pointer"""
        s = abi.Sample()
        abi.check(self.lib.zh_sample_kit_sample(self.handle, i, C.byref(s)), "zh_sample_kit_sample")
        return s

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zh_sample_kit_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


class SamplePlayer:
    def __init__(self, ctx, n_players, kit, polyphony=1, sample_rate=48000, distort=False, max_impulses=None):
        """`polyphony`: voices per player (the example has one Sampler: 1).  `max_impulses`: the most pushes one buffer may carry
        over all players (default 33 per player: one more than their queues accept)."""
        self.ctx, self.kit, self.n_players, self.polyphony = ctx, kit, int(n_players), int(polyphony)
        self.sample_rate, self.distort = float(sample_rate), bool(distort)
        self.n_voices = self.n_players * self.polyphony
        self.bank = LiveVoiceBank(ctx, self.n_players, self.polyphony, NOTE_PARAMS, NOTE_PARAMS.fields["note_on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=MAX_SPANS)
        word = lambda name: NOTE_PARAMS.fields[name][1] // 4
        self._table = self.bank.script_table(MAX_SPANS, {"sample_rate": (word("sample_rate"), "f"), "loop": (word("loop"), "u"),
                                                         "sample": (word("sample"), "u"), "channel": (word("channel"), "u")})
        self.voices = mod.Sampler(self.n_voices, ctx)
        self._params = mod.Sampler.KitParams(kit, self.sample_rate, 0, 0, False)     # every field has a span array
        self._overdrive = None
        self._frames = 0

    def push(self, player, frame, note_id, sample, rate, channel=0, loop=False):
        """keyEvent's iq.push (:121-139): scalars, or equal-length arrays in push order.  `rate`: the output rate the note is
        played at (Sampler.Params.sample_rate: the pitch; negative plays backwards, with loop)."""
        rate = np.atleast_1d(np.asarray(rate, np.float32))
        rec = np.zeros(len(rate), NOTE_PARAMS)
        rec["sample_rate"], rec["sample"], rec["channel"], rec["loop"] = rate, sample, channel, np.asarray(loop).astype(np.uint32)
        rec["note_on"] = 1                                           # the dispatcher needs one; a sample has no note-off
        self.bank.push(player, frame, note_id, rec)

    def _reserve(self, frames):
        if frames > self._frames:
            self._image = self.ctx.image(frames, self.n_voices)
            self._mix = torch.zeros((self.n_players, frames), dtype=torch.float32, device=self.ctx.device)
            self._out = torch.zeros((self.n_players, frames), dtype=torch.float32, device=self.ctx.device)
            self._frames = frames

    def paint(self, frames, distort=None):
        """one buffer -> the [n_players][frames] f32 rows, on the device (a view of a buffer the next call overwrites).  Every step
        is enqueued; nothing synchronises.  `distort`: the example's `d` key for this buffer (None: as constructed)."""
        self._reserve(frames)
        distort = self.distort if distort is None else bool(distort)
        span = zang.Span(0, frames)
        self.bank.schedule(frames, MAX_SPANS)
        img = self._image[:frames]
        self.voices.paint_kit_spans(span, [img], None, self._params, self._table, zero_first=True)
        zang.mixdownGroups(span, self._mix, img, self.polyphony, zero_first=True, ctx=self.ctx)
        # the gain and the overdrive are elementwise: the rows are an image of n_players frames x `frames` voices to them
        rows, mix = zang.Span(0, self.n_players), self._mix[:, :frames]
        zang.multiplyWithScalar(rows, mix, GAIN, ctx=self.ctx)
        if not distort:
            return mix
        if self._overdrive is None or self._overdrive.n_voices != frames:
            if self._overdrive is not None:
                self._overdrive.close()
            self._overdrive = mod.Distortion(frames, self.ctx)
        out = self._out[:, :frames]
        self._overdrive.paint(rows, [out], [], False, mod.Distortion.Params(mix, mod.Distortion.overdrive, *OVERDRIVE), zero_first=True)
        return out

    def overflows(self):
        return self.bank.overflows()

    def close(self):
        for o in (self.voices, self._overdrive, self.bank):
            if o is not None:
                o.close()
