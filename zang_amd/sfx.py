"""Sound effects: an effect kit -- K triples of curves resident on the device (zh_sfx_kit) -- and LaserPlayer, N of the reference's
laser examples (examples/example_laser.zig MainModule, :119-223) played live.  The reference hard-wires one triple of curves
(:22-38) and gets its four sounds from four scalars (:161-220); here a pushed impulse also names an effect of the kit.  Per
buffer: the pushed impulses go through one LiveVoiceBank launch (ImpulseQueue -> PolyphonyDispatcher -> Triggers) and one
zh_laser_paint_spans renders every voice's sub-spans with each impulse's effect and scalars (:149-158); with more than one
voice per player the grouped mixdown adds each player's voices in voice order.  CurvePlayer does the same for the curve voice of
examples/example_curve.zig (zh_curve_player_paint_spans), whose sounds outlive buffers."""
import ctypes as C

import numpy as np
import torch

from . import abi, modules as mod, zang
from .bank import LiveVoiceBank

# the note record: LaserPlayer.Params (:43-49) without the shared sample rate, the effect, and the note_on the dispatcher reads
NOTE_PARAMS = np.dtype([("freq_mul", "<f4"), ("carrier_mul", "<f4"), ("modulator_mul", "<f4"), ("modulator_rad", "<f4"),
                        ("effect", "<u4"), ("note_on", "<u4")])
MAX_SPANS = 34                                  # 32 impulses a buffer (the ImpulseQueue's cap) + the carried note + 1
linear, smoothstep = 0, 1                       # ZH_CURVE_FN_*

# example_laser.zig:22-38 as (t, value) pairs
DEFAULT_CARRIER = [(0.0, 1000.0), (0.1, 200.0), (0.2, 100.0)]
DEFAULT_MODULATOR = [(0.0, 1000.0), (0.1, 200.0), (0.2, 100.0)]
DEFAULT_VOLUME = [(0.0, 0.0), (0.004, 1.0), (0.2, 0.0)]


def default_effect():
    """the reference's triple as SfxKit takes an effect: (modulator, carrier, volume), each (nodes, function)"""
    return ((DEFAULT_MODULATOR, smoothstep), (DEFAULT_CARRIER, smoothstep), (DEFAULT_VOLUME, smoothstep))


# example_curve.zig:18-31 as (t, value) pairs
CURVE_EXAMPLE_CARRIER = [(0.0, 440.0), (0.5, 880.0), (1.0, 110.0), (1.5, 660.0), (2.0, 330.0), (3.9, 20.0)]
CURVE_EXAMPLE_MODULATOR = [(0.0, 110.0), (1.5, 55.0), (3.0, 220.0)]
# the curve voice's note record: CurvePlayer.Params (example_curve.zig:36-39) without the shared sample rate, the effect, and the
# note_on the dispatcher reads
CURVE_NOTE_PARAMS = np.dtype([("rel_freq", "<f4"), ("effect", "<u4"), ("note_on", "<u4")])


def curve_example_effect():
    """the pair of curves of examples/example_curve.zig as SfxKit takes an effect; the curve voice reads no volume curve"""
    return ((CURVE_EXAMPLE_MODULATOR, smoothstep), (CURVE_EXAMPLE_CARRIER, smoothstep), ([], smoothstep))


def presets():
    """the four sounds of keyEvent (:161-220): name -> (carrier_mul, modulator_mul, modulator_rad), with the variance terms
    left out (freq_mul is 1 +- 0.15 for all four; the player laser also varies modulator_mul by +- 0.05 and modulator_rad by
    +- 0.125)"""
    return {"player_laser": (2.0, 0.5, 0.5), "enemy_laser": (4.0, 0.125, 1.0), "pain": (0.5, 0.125, 1.0), "web": (1.0, 9.0, 1.0)}


def _nodes(curve):
    """[(t, value)] -> a host array of zh_curve_node {value, t}"""
    a = np.zeros((len(curve), 2), np.float32)
    for i, (t, value) in enumerate(curve):
        a[i] = (value, t)
    return a


class SfxKit:
    """`effects`: a list of (modulator, carrier, volume), each a pair ([(t, value), ...], function) with function `linear` or
    `smoothstep`; node lists of any length, 0 too, on the HOST -- the kit copies them to the device once."""

    def __init__(self, ctx, effects):
        self.ctx, self.lib = ctx, ctx.lib
        keep = []
        arr = (abi.SfxEffect * max(len(effects), 1))()
        for i, triple in enumerate(effects):
            cs = []
            for curve, function in triple:
                a = _nodes(curve)
                keep.append(a)
                cs.append(abi.SfxCurve(a.ctypes.data if len(a) else None, len(a), int(function)))
            arr[i] = abi.SfxEffect(*cs)
        self.handle = C.c_void_p()
        abi.check(self.lib.zh_sfx_kit_create(ctx.handle, arr, len(effects), C.byref(self.handle)), "zh_sfx_kit_create")
        self.count = len(effects)
        ctx._children.add(self)

    def effect(self, i):
        """entry i as an abi.SfxEffect whose `nodes` are DEVICE pointers: what zh_curve_module_params.curve takes"""
        e = abi.SfxEffect()
        abi.check(self.lib.zh_sfx_kit_effect(self.handle, i, C.byref(e)), "zh_sfx_kit_effect")
        return e

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zh_sfx_kit_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


class LaserPlayer:
    def __init__(self, ctx, n_players, kit, polyphony=1, sample_rate=48000, max_impulses=None):
        """`polyphony`: voices per player (the example has one LaserPlayer: 1, a new impulse cuts the sound off).
        `max_impulses`: the most pushes one buffer may carry over all players (default 33 per player: one more than their
        queues accept)."""
        self.ctx, self.kit, self.n_players, self.polyphony = ctx, kit, int(n_players), int(polyphony)
        self.sample_rate = float(sample_rate)
        self.n_voices = self.n_players * self.polyphony
        self.bank = LiveVoiceBank(ctx, self.n_players, self.polyphony, NOTE_PARAMS, NOTE_PARAMS.fields["note_on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=MAX_SPANS)
        word = lambda name: NOTE_PARAMS.fields[name][1] // 4
        self._table = self.bank.script_table(MAX_SPANS, {n: (word(n), "u" if n == "effect" else "f") for n, _ in mod.Laser._span_fields})
        self.voices = mod.Laser(self.n_voices, ctx)
        self._params = mod.Laser.Params(kit, self.sample_rate)       # every field has a span array
        self._frames = 0

    def push(self, player, frame, note_id, effect, freq_mul=1.0, carrier_mul=1.0, modulator_mul=1.0, modulator_rad=1.0):
        """keyEvent's iq.push (:173-215): scalars, or equal-length arrays in push order"""
        cols = [np.atleast_1d(np.asarray(x, np.float32)) for x in (freq_mul, carrier_mul, modulator_mul, modulator_rad)]
        n = max(max(len(c) for c in cols), np.atleast_1d(np.asarray(effect)).size)
        rec = np.zeros(n, NOTE_PARAMS)
        rec["freq_mul"], rec["carrier_mul"], rec["modulator_mul"], rec["modulator_rad"] = cols
        rec["effect"] = effect
        rec["note_on"] = 1                                           # the dispatcher needs one; an effect has no note-off
        self.bank.push(player, frame, note_id, rec)

    def _reserve(self, frames):
        if frames > self._frames:
            self._image = self.ctx.image(frames, self.n_voices)
            self._mix = torch.zeros((self.n_players, frames), dtype=torch.float32, device=self.ctx.device)
            self._frames = frames

    def paint(self, frames):
        """one buffer -> [n_players][frames] f32 on the device (a view of a buffer the next call overwrites).  Every step is
        enqueued; nothing synchronises."""
        self._reserve(frames)
        span = zang.Span(0, frames)
        self.bank.schedule(frames, MAX_SPANS)
        img = self._image[:frames]
        self.voices.paint_spans(span, [img], None, self._params, self._table, zero_first=True)
        if self.polyphony == 1:
            return img.t()
        zang.mixdownGroups(span, self._mix, img, self.polyphony, zero_first=True, ctx=self.ctx)
        return self._mix[:, :frames]

    def overflows(self):
        return self.bank.overflows()

    def close(self):
        for o in (self.voices, self.bank):
            if o is not None:
                o.close()


class CurvePlayer:
    """N of the reference's curve examples (examples/example_curve.zig MainModule, :98-144) played live.  Per buffer: the pushed
    impulses go through one LiveVoiceBank launch and one zh_curve_player_paint_spans renders every voice's sub-spans with each
    impulse's rel_freq and effect (:126-129).  A sound runs for as long as its curves (the example's: 3.9 s): the voices carry it
    from buffer to buffer."""

    def __init__(self, ctx, n_players, kit, polyphony=1, sample_rate=48000, sync=False, max_impulses=None):
        """`polyphony`: voices per player (the example has one CurvePlayer: 1, a new impulse restarts the sound).  `sync`: the
        carrier's frequency image (the example's output_sync_oscilloscope) is painted too.  `max_impulses`: the most pushes one
        buffer may carry over all players (default 33 per player: one more than their queues accept)."""
        self.ctx, self.kit, self.n_players, self.polyphony = ctx, kit, int(n_players), int(polyphony)
        self.sample_rate, self.sync = float(sample_rate), bool(sync)
        self.n_voices = self.n_players * self.polyphony
        self.bank = LiveVoiceBank(ctx, self.n_players, self.polyphony, CURVE_NOTE_PARAMS, CURVE_NOTE_PARAMS.fields["note_on"][1],
                                  33 * self.n_players if max_impulses is None else int(max_impulses), rows=MAX_SPANS)
        word = lambda name: CURVE_NOTE_PARAMS.fields[name][1] // 4
        self._table = self.bank.script_table(MAX_SPANS, {"rel_freq": (word("rel_freq"), "f"), "effect": (word("effect"), "u")})
        self.voices = mod.CurveVoice(self.n_voices, ctx)
        self._params = mod.CurveVoice.Params(kit, self.sample_rate)   # every field has a span array
        self._frames = 0

    def push(self, player, frame, note_id, effect=0, rel_freq=1.0):
        """keyEvent's iq.push (:135-138): scalars, or equal-length arrays in push order"""
        rel_freq = np.atleast_1d(np.asarray(rel_freq, np.float32))
        rec = np.zeros(max(len(rel_freq), np.atleast_1d(np.asarray(effect)).size), CURVE_NOTE_PARAMS)
        rec["rel_freq"] = rel_freq
        rec["effect"] = effect
        rec["note_on"] = 1                                           # the dispatcher needs one; the sound has no note-off
        self.bank.push(player, frame, note_id, rec)

    def _reserve(self, frames):
        if frames > self._frames:
            self._image = self.ctx.image(frames, self.n_voices)
            self._sync = self.ctx.image(frames, self.n_voices) if self.sync else None
            self._mix = torch.zeros((self.n_players, frames), dtype=torch.float32, device=self.ctx.device)
            self._frames = frames

    def paint(self, frames):
        """one buffer -> [n_players][frames] f32 on the device, or with sync=True (that, the frequency image [n_voices][frames])
        (views of buffers the next call overwrites).  Every step is enqueued; nothing synchronises."""
        self._reserve(frames)
        span = zang.Span(0, frames)
        self.bank.schedule(frames, MAX_SPANS)
        img = self._image[:frames]
        sync = self._sync[:frames] if self.sync else None
        self.voices.paint_spans(span, [img, sync], None, self._params, self._table, zero_first=True)
        if self.polyphony == 1:
            out = img.t()
        else:
            zang.mixdownGroups(span, self._mix, img, self.polyphony, zero_first=True, ctx=self.ctx)
            out = self._mix[:, :frames]
        return (out, sync.t()) if self.sync else out

    def overflows(self):
        return self.bank.overflows()

    def close(self):
        for o in (self.voices, self.bank):
            if o is not None:
                o.close()
