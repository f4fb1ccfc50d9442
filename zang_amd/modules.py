"""Host-side mirror of the reference's `modules` namespace (src/modules.zig:1-13) for the
paint path: each class keeps the Zig module's interface --

    num_outputs, num_temps, Params, init(), paint(span, outputs, temps, note_id_changed, params)

(src/modules/SineOsc.zig:8-31) -- but one instance holds n_voices independent module states
on the device and one paint() call renders all of them through libzang_hip.so.
`outputs`/`temps` are lists of [frame][voice] float32 CUDA tensors; scalar params may be
Python floats (broadcast) or float32 CUDA tensors [n_voices]; `note_id_changed`/`note_on`
may be bools or uint8/bool CUDA tensors [n_voices].
"""
import ctypes as C
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from . import abi
from .runtime import as_bool, as_buf, as_f32, as_u32, default_context


def _bufarray(tensors):
    if not tensors:
        return None
    arr = (abi.Buf * len(tensors))(*[as_buf(t) for t in tensors])
    return arr


def _np_state(ctype, n):
    return np.zeros(n, dtype=np.dtype(ctype))


class _Module:
    num_outputs = 1
    num_temps = 0
    _prefix = ""
    _state_ctype = None

    def __init__(self, n_voices, ctx=None, *create_args):
        self.ctx = ctx or default_context()
        self.n_voices = int(n_voices)
        self.lib = self.ctx.lib
        h = C.c_void_p()
        create = getattr(self.lib, f"zh_{self._prefix}_create")
        abi.check(create(self.ctx.handle, self.n_voices, *create_args, C.byref(h)), f"zh_{self._prefix}_create")
        self.handle = h
        self.ctx._children.add(self)

    @classmethod
    def init(cls, n_voices, ctx=None):
        return cls(n_voices, ctx)

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.lib, f"zh_{self._prefix}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # state as a numpy structured array mirroring the Zig struct fields
    def state(self):
        st = _np_state(self._state_ctype, self.n_voices)
        abi.check(getattr(self.lib, f"zh_{self._prefix}_get_state")(self.handle, st.ctypes.data), "get_state")
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.dtype(self._state_ctype))
        assert st.shape == (self.n_voices,)
        abi.check(getattr(self.lib, f"zh_{self._prefix}_set_state")(self.handle, st.ctypes.data), "set_state")

    def _paint(self, span, outputs, temps, note_id_changed, cparams, zero_first, extra_flags=0):
        outs = _bufarray(outputs)
        tmps = _bufarray(temps)
        fn = getattr(self.lib, f"zh_{self._prefix}_paint")
        rc = fn(self.handle, span.start, span.end, outs, tmps, as_bool(note_id_changed), C.byref(cparams),
                (abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD) | extra_flags)
        abi.check(rc, f"zh_{self._prefix}_paint")

    # zh_<module>_paint_spans: the module's span fields in the C order (ZH_<MODULE>_SPAN_*), each (name, kind) with kind
    # "constant" (an `f` array), "boolean" / "tag" (a `u` array) or "curve" (both: the tag in `u`, the duration in `f`)
    _span_fields = ()

    @classmethod
    def span_spec(cls):
        """the spec of a zang_amd.script.ScriptSpanTable for this module: [(field, kind, None)]"""
        return [(n, k, None) for n, k in cls._span_fields]

    @classmethod
    def span_table(cls, count, start, end, note_id_changed, values=None):
        """A per-voice sub-span table for paint_spans: count [V], start / end / note_id_changed [K][V] (host arrays), and
        `values` {field: (f [K][V] or None, u [K][V] or None)} for the fields that vary per sub-span (span_spec())."""
        from .script import ScriptSpanTable
        return ScriptSpanTable(cls.span_spec(), count, start, end, note_id_changed, values)

    def paint_spans(self, span, outputs, temps, params, table, zero_first=False):
        """The reference's Trigger loop for every voice in one launch (zh_<module>_paint_spans): voice v runs paint(sub-span k,
        ..., note_id_changed[k][v], params with the table's per-sub-span values) for each of its sub-spans in `table` (a
        zang_amd.script.ScriptSpanTable, e.g. from span_table()).  `params`: the Params paint() takes, for every field the
        table holds no array for.  Frames outside a voice's sub-spans are left alone, or zeroed with zero_first=True."""
        rc = self._paint_spans(span, outputs, temps, params, table, abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, f"zh_{self._prefix}_paint_spans")

    def _paint_spans(self, span, outputs, temps, params, table, flags, span_params=None):
        """-> the return code; `span_params`: a ctypes ScriptSpanParam array to pass instead of the table's (the error tests)"""
        cp = self._cparams(params)
        tb, sp = table.device(self.ctx.device, [n for n, _ in self._span_fields])
        if span_params is not None:
            sp = span_params
        fn = getattr(self.lib, f"zh_{self._prefix}_paint_spans")
        rc = fn(self.handle, span.start, span.end, _bufarray(outputs), _bufarray(temps), C.byref(cp), sp, C.byref(tb), flags)
        self._keep = (cp, outputs, table)
        return rc

    def _paint_batch(self, span, images, cparams, zero_first, extra_flags=0):
        outs = _bufarray(images)
        fn = getattr(self.lib, f"zh_{self._prefix}_paint_batch")
        rc = fn(self.handle, span.start, span.end, outs, len(images), C.byref(cparams),
                (abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD) | extra_flags)
        abi.check(rc, f"zh_{self._prefix}_paint_batch")


class SineOsc(_Module):
    """src/modules/SineOsc.zig"""
    _prefix = "sineosc"
    _state_ctype = abi.SineOscState

    @dataclass
    class Params:
        sample_rate: float
        freq: Any   # zang.constant(...) | zang.buffer(...)
        phase: Any

    _span_fields = (("freq", "constant"), ("phase", "constant"))

    @staticmethod
    def _cparams(params):
        return abi.SineOscParams(params.sample_rate, 0, params.freq, params.phase)

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT -- the sine in f32 (within 1e-5 of the peak, measured 3e-7); the phase state stays exact."""
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first, abi.PAINT_TOLERANT if tolerant else 0)


class PulseOsc(_Module):
    """src/modules/PulseOsc.zig"""
    _prefix = "pulseosc"
    _state_ctype = abi.PulseOscState

    @dataclass
    class Params:
        sample_rate: float
        freq: Any
        color: Any

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, params_unchanged=False):
        """`params_unchanged`: the caller states that `params` (per-voice array contents included) are what the
        previous paint of this module got (ZH_PAINT_PARAMS_UNCHANGED, include/zang_hip.h); same bits either way."""
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first, abi.PAINT_PARAMS_UNCHANGED if params_unchanged else 0)

    _span_fields = (("freq", "constant"), ("color", "constant"))

    @staticmethod
    def _cparams(params):
        return abi.PulseOscParams(params.sample_rate, 0, params.freq, as_f32(params.color))

    def paint_batch(self, span, images, params, zero_first=False, params_unchanged=False):
        """len(images) consecutive paint calls with the same span and params, call b into images[b], as one launch
        when the frequency is constant (zh_pulseosc_paint_batch)."""
        cp = abi.PulseOscParams(params.sample_rate, 0, params.freq, as_f32(params.color))
        self._paint_batch(span, images, cp, zero_first, abi.PAINT_PARAMS_UNCHANGED if params_unchanged else 0)


class TriSawOsc(_Module):
    """src/modules/TriSawOsc.zig"""
    _prefix = "trisawosc"
    _state_ctype = abi.TriSawOscState

    @dataclass
    class Params:
        sample_rate: float
        freq: Any
        color: Any

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, params_unchanged=False):
        """`params_unchanged`: the caller states that `params` (per-voice array contents included) are what the
        previous paint of this module got (ZH_PAINT_PARAMS_UNCHANGED, include/zang_hip.h); same bits either way."""
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first, abi.PAINT_PARAMS_UNCHANGED if params_unchanged else 0)

    _span_fields = (("freq", "constant"), ("color", "constant"))

    @staticmethod
    def _cparams(params):
        return abi.TriSawOscParams(params.sample_rate, 0, params.freq, as_f32(params.color))

    def paint_batch(self, span, images, params, zero_first=False, params_unchanged=False):
        """len(images) consecutive paint calls with the same span and params, call b into images[b], as one launch
        when the frequency is constant (zh_trisawosc_paint_batch)."""
        cp = abi.TriSawOscParams(params.sample_rate, 0, params.freq, as_f32(params.color))
        self._paint_batch(span, images, cp, zero_first, abi.PAINT_PARAMS_UNCHANGED if params_unchanged else 0)


class Noise(_Module):
    """src/modules/Noise.zig.  `first_seed` is the global index of voice 0: voice v is seeded
    like the (first_seed+v)-th Noise.init() of a process (Noise.zig:9,26)."""
    _prefix = "noise"
    _state_ctype = abi.NoiseState
    white, pink = abi.NOISE_WHITE, abi.NOISE_PINK

    @dataclass
    class Params:
        color: int

    def __init__(self, n_voices, ctx=None, first_seed=0):
        super().__init__(n_voices, ctx, C.c_uint64(first_seed))

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT -- pink noise at few voices: the taps as chunks at once over exactly generated white
        noise (1e-5 of the voice's peak); white noise and the generator's state are always exact."""
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first, abi.PAINT_TOLERANT if tolerant else 0)

    _span_fields = (("color", "tag"),)

    @staticmethod
    def _cparams(params):
        return abi.NoiseParams(params.color)


class Envelope(_Module):
    """src/modules/Envelope.zig over src/zang/painter.zig"""
    _prefix = "envelope"
    _state_ctype = abi.EnvelopeState

    @dataclass
    class Params:
        sample_rate: float
        attack: Any     # zang.PaintCurve.*
        decay: Any
        release: Any
        sustain_volume: Any
        note_on: Any

    _span_fields = (("attack", "curve"), ("decay", "curve"), ("release", "curve"), ("sustain_volume", "constant"), ("note_on", "boolean"))

    @staticmethod
    def _cparams(params):
        return abi.EnvelopeParams(params.sample_rate, 0, params.attack, params.decay, params.release,
                                  as_f32(params.sustain_volume), as_bool(params.note_on))

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first)


class Gate(_Module):
    """src/modules/Gate.zig (stateless)"""
    _prefix = "gate"

    @dataclass
    class Params:
        note_on: Any

    _span_fields = (("note_on", "boolean"),)

    @staticmethod
    def _cparams(params):
        return abi.GateParams(as_bool(params.note_on))

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first)

    def state(self):
        raise AttributeError("Gate has no state")


class Filter(_Module):
    """src/modules/Filter.zig"""
    _prefix = "filter"
    _state_ctype = abi.FilterState
    bypass, low_pass, band_pass, high_pass, notch, all_pass = range(6)

    @dataclass
    class Params:
        input: Any
        type: int
        cutoff: Any
        res: Any

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT (opt-in, 1e-5 of the signal's peak instead of bits; include/zang_hip.h)."""
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first, abi.PAINT_TOLERANT if tolerant else 0)

    _span_fields = (("type", "tag"), ("cutoff", "constant"), ("res", "constant"))

    @staticmethod
    def _cparams(params):
        return abi.FilterParams(as_buf(params.input), params.type, 0, params.cutoff, params.res)

    @staticmethod
    def cutoffFromFrequency(frequency, sample_rate, ctx=None):
        """Filter.cutoffFromFrequency (Filter.zig:20-23) for a float32 CUDA tensor of frequencies."""
        import torch
        c = ctx or default_context()
        out = torch.empty_like(frequency)
        abi.check(c.lib.zh_filter_cutoff_from_frequency(c.handle, frequency.numel(), out.data_ptr(),
                                                        frequency.data_ptr(), float(sample_rate)), "cutoff")
        return out


class Sampler(_Module):
    """src/modules/Sampler.zig"""
    _prefix = "sampler"
    _state_ctype = abi.SamplerState
    unsigned8, signed16_lsb, signed24_lsb, signed32_lsb = range(4)

    @dataclass
    class Sample:
        num_channels: int
        sample_rate: int
        format: int
        data: Any       # uint8 CUDA tensor

    @dataclass
    class Params:
        sample_rate: Any
        sample: Any
        channel: int
        loop: bool

    _span_fields = (("sample_rate", "constant"), ("loop", "boolean"))

    @staticmethod
    def _cparams(params):
        s = params.sample
        cs = abi.Sample(s.num_channels, s.sample_rate, s.format, 0, s.data.data_ptr(), s.data.numel())
        return abi.SamplerParams(as_f32(params.sample_rate), cs, params.channel, 1 if params.loop else 0, 0)

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first)

    # ---- over a sample kit (zang_amd.samplekit.SampleKit): the sample and the channel are per-voice / per-note values too
    @dataclass
    class KitParams:
        kit: Any            # SampleKit
        sample_rate: Any    # float, or float32 CUDA tensor [n_voices]
        sample: Any         # int, or int32 CUDA tensor [n_voices]: the index into the kit
        channel: Any = 0    # int, or int32 CUDA tensor [n_voices]
        loop: Any = False   # bool, or uint8 / bool CUDA tensor [n_voices]

    _kit_span_fields = (("sample_rate", "constant"), ("loop", "boolean"), ("sample", "tag"), ("channel", "tag"))

    @classmethod
    def kit_span_table(cls, count, start, end, note_id_changed, values=None):
        """span_table() for paint_kit_spans: `values` {field of _kit_span_fields: (f [K][V] or None, u [K][V] or None)}"""
        from .script import ScriptSpanTable
        return ScriptSpanTable([(n, k, None) for n, k in cls._kit_span_fields], count, start, end, note_id_changed, values)

    @staticmethod
    def _kit_cparams(params):
        return abi.SamplerKitParams(as_f32(params.sample_rate), as_bool(params.loop), as_u32(params.sample), as_u32(params.channel),
                                    params.kit.handle)

    def paint_kit(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        """n Sampler instances, each with its own sample, channel, rate and loop flag (KitParams), in one paint (zh_sampler_paint_kit)"""
        cp = self._kit_cparams(params)
        rc = self.lib.zh_sampler_paint_kit(self.handle, span.start, span.end, _bufarray(outputs), _bufarray(temps), as_bool(note_id_changed),
                                           C.byref(cp), abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, "zh_sampler_paint_kit")

    def paint_kit_spans(self, span, outputs, temps, params, table, zero_first=False):
        """paint_spans with the note's sample and channel among the per-sub-span values (zh_sampler_paint_kit_spans): `params` a
        KitParams for the fields `table` holds no array for; `table` from kit_span_table() or a voice bank's script_table()."""
        rc = self._paint_kit_spans(span, outputs, temps, params, table, abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, "zh_sampler_paint_kit_spans")

    def _paint_kit_spans(self, span, outputs, temps, params, table, flags, span_params=None):
        """-> the return code; `span_params`: a ctypes ScriptSpanParam array to pass instead of the table's (the error tests)"""
        cp = self._kit_cparams(params)
        tb, sp = table.device(self.ctx.device, [n for n, _ in self._kit_span_fields])
        if span_params is not None:
            sp = span_params
        rc = self.lib.zh_sampler_paint_kit_spans(self.handle, span.start, span.end, _bufarray(outputs), _bufarray(temps), C.byref(cp), sp,
                                                 C.byref(tb), flags)
        self._keep = (cp, outputs, table, params)
        return rc


class Decimator(_Module):
    """src/modules/Decimator.zig"""
    _prefix = "decimator"
    _state_ctype = abi.DecimatorState

    @dataclass
    class Params:
        sample_rate: float
        input: Any
        fake_sample_rate: Any

    _span_fields = (("fake_sample_rate", "constant"),)

    @staticmethod
    def _cparams(params):
        return abi.DecimatorParams(params.sample_rate, 0, as_buf(params.input), as_f32(params.fake_sample_rate))

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first)

    def _paint_groups(self, span, dst, src, group_voices, sample_rate, modes, flags):
        """-> the return code of zh_decimator_paint_groups"""
        return self.lib.zh_decimator_paint_groups(self.handle, span.start, span.end, dst.data_ptr(), dst.stride(0), as_buf(src), group_voices,
                                                  float(sample_rate), modes.data_ptr(), flags)

    def paint_groups(self, span, dst, src, group_voices, sample_rate, modes, zero_first=False):
        """The decimated group mix (zh_decimator_paint_groups), this module one voice per group: every group of `group_voices`
        consecutive voices of `src` added in voice order from +0, then through its Decimator -- or straight on where its mode is a
        bypass -- onto dst[g] (float32 CUDA tensor [groups, >= span.end]).  `modes`: a CUDA uint8 tensor holding [groups]
        abi.GroupDecimation records (group_modes())."""
        assert dst.dtype == torch.float32 and dst.dim() == 2 and dst.stride(1) == 1 and dst.shape[0] == self.n_voices
        assert modes.is_cuda and modes.is_contiguous() and modes.numel() * modes.element_size() == self.n_voices * C.sizeof(abi.GroupDecimation)
        abi.check(self._paint_groups(span, dst, src, group_voices, sample_rate, modes, abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD),
                  "zh_decimator_paint_groups")

    def group_modes(self, fake_sample_rates, bypass):
        """[groups] rates and bypass flags -> the device array paint_groups takes (a copy from the host)"""
        rec = np.zeros(self.n_voices, np.dtype(abi.GroupDecimation))
        rec["fake_sample_rate"], rec["bypass"] = fake_sample_rates, bypass
        return torch.from_numpy(rec.view(np.uint8).copy()).to(self.ctx.device)


class Distortion(_Module):
    """src/modules/Distortion.zig (stateless)"""
    _prefix = "distortion"
    overdrive, clip = 0, 1

    @dataclass
    class Params:
        input: Any
        type: int
        ingain: Any
        outgain: Any
        offset: Any

    _span_fields = (("type", "tag"), ("ingain", "constant"), ("outgain", "constant"), ("offset", "constant"))

    @staticmethod
    def _cparams(params):
        return abi.DistortionParams(as_buf(params.input), params.type, 0, as_f32(params.ingain),
                                    as_f32(params.outgain), as_f32(params.offset))

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first)

    def state(self):
        raise AttributeError("Distortion has no state")


class Curve(_Module):
    """src/modules/Curve.zig.  `curve` is a float32 CUDA tensor [n_nodes, 2] of (value, t) rows
    (zang.CurveNode), shared by all voices."""
    _prefix = "curve_module"
    _state_ctype = abi.CurveModuleState
    linear, smoothstep = 0, 1

    @dataclass
    class Params:
        sample_rate: float
        function: int
        curve: Any

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        c = params.curve
        assert c.is_cuda and c.dim() == 2 and c.shape[1] == 2 and c.is_contiguous()
        cp = abi.CurveModuleParams(params.sample_rate, params.function, c.data_ptr(), c.shape[0])
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first)


class Cycle(_Module):
    """src/modules/Cycle.zig"""
    _prefix = "cycle"
    _state_ctype = abi.CycleState

    @dataclass
    class Params:
        sample_rate: float
        speed: Any

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, abi.CycleParams(params.sample_rate, 0, params.speed), zero_first)


class Portamento(_Module):
    """src/modules/Portamento.zig"""
    _prefix = "portamento"
    _state_ctype = abi.PortamentoState

    @dataclass
    class Params:
        sample_rate: float
        curve: Any
        goal: Any
        note_on: Any
        prev_note_on: Any

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        cp = abi.PortamentoParams(params.sample_rate, 0, params.curve, as_f32(params.goal), as_bool(params.note_on),
                                  as_bool(params.prev_note_on))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first)


class NiceInstrument(_Module):
    """examples/modules.zig:189-248 as one fused kernel (temps are accepted and ignored)."""
    _prefix = "nice"
    _state_ctype = abi.NiceState
    num_temps = 2

    @dataclass
    class Params:
        sample_rate: float
        freq: Any
        note_on: Any

    def __init__(self, n_voices, color, ctx=None):
        self._color = as_f32(color)
        super().__init__(n_voices, ctx, self._color)

    @classmethod
    def init(cls, n_voices, color, ctx=None):
        return cls(n_voices, color, ctx)

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT -- few voices: the filter as chunks at once (1e-5 of the voice's peak); oscillator and
        envelope, and their states, stay exact."""
        cp = abi.NiceParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first, abi.PAINT_TOLERANT if tolerant else 0)

    def paint_spans(self, span, outputs, temps, sample_rate, table, zero_first=False):
        """Render every voice's Trigger sub-spans of this buffer in one launch (zang_amd.spans.SpanTable)."""
        rc = self.lib.zh_nice_paint_spans(self.handle, span.start, span.end, _bufarray(outputs), _bufarray(temps),
                                          float(sample_rate), C.byref(table.c), abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, "zh_nice_paint_spans")

    def paint_mix(self, span, mix, note_id_changed, params, zero_first=False, tolerant=False):
        """The fused chain followed by the voice mixdown into mix[frames] (device float32)."""
        cp = abi.NiceParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on))
        rc = self.lib.zh_nice_paint_mix(self.handle, span.start, span.end, mix.data_ptr(), as_bool(note_id_changed),
                                        C.byref(cp), (abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD) | (abi.PAINT_TOLERANT if tolerant else 0))
        abi.check(rc, "zh_nice_paint_mix")

    def paint_mix_stereo(self, span, mix_left, mix_right, gain_left, gain_right, note_id_changed, params, zero_first=False, tolerant=False):
        """Two channels: mix_c[f] (+)= sum over voices of voice[f] * gain_c[voice] (examples/example_stereo.zig:92-98)."""
        cp = abi.NiceParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on))
        rc = self.lib.zh_nice_paint_mix_stereo(self.handle, span.start, span.end, mix_left.data_ptr(), mix_right.data_ptr(),
                                               as_f32(gain_left), as_f32(gain_right), as_bool(note_id_changed), C.byref(cp),
                                               (abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD) | (abi.PAINT_TOLERANT if tolerant else 0))
        abi.check(rc, "zh_nice_paint_mix_stereo")

    def paint_mix_stereo_batch(self, span, mix_lefts, mix_rights, gain_left, gain_right, note_id_changeds, paramses, zero_first=False, tolerant=False):
        """len(paramses) consecutive paint_mix_stereo calls in ONE launch (zh_nice_paint_mix_stereo_batch): call b with
        paramses[b] / note_id_changeds[b] into mix_lefts[b] / mix_rights[b]; same bits as the separate calls.
        `tolerant`: the kernel with multiply-adds fused (within 1e-5 of the voices' peaks, not the reference's bits)."""
        n = len(paramses)
        assert n == len(mix_lefts) == len(mix_rights) == len(note_id_changeds) and n <= 16
        ls = (C.c_void_p * n)(*[t.data_ptr() for t in mix_lefts])
        rs = (C.c_void_p * n)(*[t.data_ptr() for t in mix_rights])
        nics = (abi.Bool * n)(*[as_bool(x) for x in note_id_changeds])
        cps = (abi.NiceParams * n)(*[abi.NiceParams(p.sample_rate, 0, as_f32(p.freq), as_bool(p.note_on)) for p in paramses])
        rc = self.lib.zh_nice_paint_mix_stereo_batch(self.handle, span.start, span.end, n, ls, rs, as_f32(gain_left), as_f32(gain_right),
                                                     nics, cps, (abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD) | (abi.PAINT_TOLERANT if tolerant else 0))
        abi.check(rc, "zh_nice_paint_mix_stereo_batch")


class SimpleDelay(_Module):
    """examples/modules.zig:341-386 over zang.Delay(delay_samples) (src/zang/delay.zig)."""
    _prefix = "delay"

    @dataclass
    class Params:
        input: Any

    def __init__(self, n_voices, delay_samples, ctx=None):
        self.delay_samples = int(delay_samples)
        super().__init__(n_voices, ctx, C.c_uint32(self.delay_samples))

    @classmethod
    def init(cls, n_voices, delay_samples, ctx=None):
        return cls(n_voices, delay_samples, ctx)

    def reset(self):
        abi.check(self.lib.zh_delay_reset(self.handle), "zh_delay_reset")

    def state(self):
        rings = np.zeros((self.n_voices, self.delay_samples), np.float32)
        index = np.zeros(self.n_voices, np.uint32)
        abi.check(self.lib.zh_delay_get_state(self.handle, rings.ctypes.data, index.ctypes.data), "get_state")
        return rings, index

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, abi.DelayParams(as_buf(params.input)), zero_first)


class FilteredEchoes(_Module):
    """examples/modules.zig:390-461."""
    _prefix = "filtered_echoes"
    num_temps = 2

    @dataclass
    class Params:
        input: Any
        feedback_volume: Any
        cutoff: Any

    def __init__(self, n_voices, delay_samples, ctx=None):
        self.delay_samples = int(delay_samples)
        super().__init__(n_voices, ctx, C.c_uint32(self.delay_samples))

    @classmethod
    def init(cls, n_voices, delay_samples, ctx=None):
        return cls(n_voices, delay_samples, ctx)

    def reset(self):
        abi.check(self.lib.zh_filtered_echoes_reset(self.handle), "reset")

    def state(self):
        rings = np.zeros((self.n_voices, self.delay_samples), np.float32)
        index = np.zeros(self.n_voices, np.uint32)
        flt = np.zeros(self.n_voices, dtype=np.dtype(abi.FilterState))
        abi.check(self.lib.zh_filtered_echoes_get_state(self.handle, rings.ctypes.data, index.ctypes.data, flt.ctypes.data), "get_state")
        return rings, index, flt

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT -- few voices: pieces of <= delay_samples frames, the filter of each as chunks at once
        (1e-5 of the voice's peak; include/zang_hip.h)."""
        cp = abi.FilteredEchoesParams(as_buf(params.input), as_f32(params.feedback_volume), as_f32(params.cutoff))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first, abi.PAINT_TOLERANT if tolerant else 0)


class StereoEchoes(_Module):
    """examples/modules.zig:464-525 as one kernel: the dry input to both outputs, SimpleDelay(main_delay / 2), FilteredEchoes(main_delay)
    to the left, a second SimpleDelay(main_delay / 2) to the right.  outputs = [left, right]; the reference's four temps are not needed.
    Input and the two outputs must not share memory."""
    _prefix = "stereo_echoes"
    num_outputs = 2
    num_temps = 4

    @dataclass
    class Params:
        input: Any
        feedback_volume: Any
        cutoff: Any

    def __init__(self, n_voices, main_delay, ctx=None):
        self.main_delay = int(main_delay)
        self.half_delay = self.main_delay // 2
        super().__init__(n_voices, ctx, C.c_uint32(self.main_delay))

    @classmethod
    def init(cls, n_voices, main_delay, ctx=None):
        return cls(n_voices, main_delay, ctx)

    def reset(self):
        """the three delays; the filter keeps its state (:488-492, :408-410)"""
        abi.check(self.lib.zh_stereo_echoes_reset(self.handle), "zh_stereo_echoes_reset")

    def state(self):
        """(rings0, idx0, rings1, idx1, rings_e, idx_e, filter): rings voice-major [n_voices][ring length]"""
        n = self.n_voices
        r0 = np.zeros((n, self.half_delay), np.float32); r1 = np.zeros((n, self.half_delay), np.float32)
        re = np.zeros((n, self.main_delay), np.float32)
        i0, i1, ie = (np.zeros(n, np.uint32) for _ in range(3))
        flt = np.zeros(n, dtype=np.dtype(abi.FilterState))
        abi.check(self.lib.zh_stereo_echoes_get_state(self.handle, r0.ctypes.data, i0.ctypes.data, r1.ctypes.data, i1.ctypes.data,
                                                      re.ctypes.data, ie.ctypes.data, flt.ctypes.data), "zh_stereo_echoes_get_state")
        return r0, i0, r1, i1, re, ie, flt

    def set_state(self, rings0, idx0, rings1, idx1, rings_e, idx_e, flt):
        n = self.n_voices
        r0 = np.ascontiguousarray(rings0, np.float32); r1 = np.ascontiguousarray(rings1, np.float32)
        re = np.ascontiguousarray(rings_e, np.float32)
        assert r0.shape == r1.shape == (n, self.half_delay) and re.shape == (n, self.main_delay)
        i0, i1, ie = (np.ascontiguousarray(i, np.uint32) for i in (idx0, idx1, idx_e))
        assert i0.shape == i1.shape == ie.shape == (n,)
        flt = np.ascontiguousarray(flt, dtype=np.dtype(abi.FilterState))
        assert flt.shape == (n,)
        abi.check(self.lib.zh_stereo_echoes_set_state(self.handle, r0.ctypes.data, i0.ctypes.data, r1.ctypes.data, i1.ctypes.data,
                                                      re.ctypes.data, ie.ctypes.data, flt.ctypes.data), "zh_stereo_echoes_set_state")

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True is refused (ZH_ERR_UNSUPPORTED): the module has exact forms only."""
        cp = abi.StereoEchoesParams(as_buf(params.input), as_f32(params.feedback_volume), as_f32(params.cutoff))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first, abi.PAINT_TOLERANT if tolerant else 0)


class NoiseFilter(_Module):
    """Noise -> Filter as one fused kernel (examples/example_stereo.zig:71-82; BASELINE config 3)."""
    _prefix = "noise_filter"
    _state_ctype = abi.NoiseFilterState
    num_temps = 1

    @dataclass
    class Params:
        color: int
        type: int
        cutoff: Any
        res: Any

    def __init__(self, n_voices, ctx=None, first_seed=0):
        super().__init__(n_voices, ctx, C.c_uint64(first_seed))

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT (opt-in, 1e-5 of the signal's peak instead of bits; include/zang_hip.h)."""
        cp = abi.NoiseFilterParams(params.color, params.type, as_f32(params.cutoff), as_f32(params.res))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first, abi.PAINT_TOLERANT if tolerant else 0)


class PMOscInstrument(_Module):
    """examples/modules.zig:80-128 (PhaseModOscillator :6-77 inside) as one fused kernel."""
    _prefix = "pmosc"
    _state_ctype = abi.PMOscState
    num_temps = 3

    @dataclass
    class Params:
        sample_rate: float
        freq: Any
        note_on: Any

    def __init__(self, n_voices, release_duration, ctx=None):
        self._rel = as_f32(release_duration)
        super().__init__(n_voices, ctx, self._rel)

    @classmethod
    def init(cls, n_voices, release_duration, ctx=None):
        return cls(n_voices, release_duration, ctx)

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """tolerant=True: ZH_PAINT_TOLERANT -- the carrier's sine in f32; phases and envelope state stay exact."""
        cp = abi.PMOscParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first, abi.PAINT_TOLERANT if tolerant else 0)

    def paint_spans(self, span, outputs, temps, sample_rate, table, zero_first=False):
        """Render every voice's Trigger sub-spans of this buffer in one launch (zang_amd.spans.SpanTable)."""
        rc = self.lib.zh_pmosc_paint_spans(self.handle, span.start, span.end, _bufarray(outputs), _bufarray(temps),
                                           float(sample_rate), C.byref(table.c), abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, "zh_pmosc_paint_spans")


class FMInstrument(_Module):
    """examples/example_fmsynth.zig:22-356: the OPL-style two-operator FM Instrument (modulator + carrier Operator, each an
    Oscillator with feedback and four waveforms times volume, tremolo and a cubed Envelope) as one fused kernel.
    `group` consecutive voices form one instrument (a synth's polyphony): instrument v // group selects the patch and the
    column of the two LFO images ([frame][n_instruments])."""
    _prefix = "fm"
    _state_ctype = abi.FMState
    num_temps = 3

    @dataclass
    class Params:
        sample_rate: float
        tremolo_input: Any
        vibrato_input: Any
        freq: Any
        note_on: Any

    def __init__(self, n_voices, ctx=None, group=1):
        self.group = int(group)
        super().__init__(n_voices, ctx, C.c_uint32(self.group))
        self.n_instruments = -(-self.n_voices // self.group)

    @classmethod
    def init(cls, n_voices, ctx=None, group=1):
        return cls(n_voices, ctx, group)

    @staticmethod
    def default_patch():
        """the current_values of parameters[0..21] (:376-397), indexed by abi.FM_*"""
        p = abi.FMPatch()
        abi.check(abi.load().zh_fm_patch_default(C.byref(p)), "zh_fm_patch_default")
        return list(p.value)

    def set_patches(self, patches):
        """`patches`: one list of 22 values (every instrument) or one per instrument.  A value outside its num_values is
        refused and nothing changes."""
        patches = np.ascontiguousarray(patches, dtype=np.uint32)
        if patches.ndim == 1:
            patches = patches[None, :]
        assert patches.ndim == 2 and patches.shape[1] == abi.FM_PATCH_VALUES, patches.shape
        abi.check(self.lib.zh_fm_set_patches(self.handle, patches.ctypes.data, patches.shape[0]), "zh_fm_set_patches")

    @staticmethod
    def _flags(zero_first, split):
        return (abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD) | (abi.FM_SPLIT_OPERATORS if split else 0)

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, split=False):
        """split=True (ZH_FM_SPLIT_OPERATORS): outputs[0] has 2 * n_voices columns -- 2v: what the modulator adds to the
        output (nothing in algorithm 1), 2v + 1: what the carrier adds."""
        cp = abi.FMParams(params.sample_rate, 0, as_buf(params.tremolo_input), as_buf(params.vibrato_input), as_f32(params.freq),
                          as_bool(params.note_on))
        self._paint(span, outputs, temps, note_id_changed, cp, zero_first, abi.FM_SPLIT_OPERATORS if split else 0)

    def paint_spans(self, span, outputs, temps, sample_rate, tremolo_input, vibrato_input, table, zero_first=False, split=False):
        """The synth's Trigger loop (:457-496) for every voice in one launch (zang_amd.spans.SpanTable, or a voice bank's)."""
        rc = self.lib.zh_fm_paint_spans(self.handle, span.start, span.end, _bufarray(outputs), _bufarray(temps), float(sample_rate),
                                        as_buf(tremolo_input), as_buf(vibrato_input), C.byref(table.c), self._flags(zero_first, split))
        abi.check(rc, "zh_fm_paint_spans")


class Laser(_Module):
    """examples/example_laser.zig:40-117: LaserPlayer -- three Curves (modulator frequency, carrier frequency, volume) driving
    a phase-modulated pair of SineOscs -- as one fused kernel.  The curves come from an effect kit (zang_amd.sfx.SfxKit); the
    effect index is a per-voice / per-note value beside the four scalars."""
    _prefix = "laser"
    _state_ctype = abi.LaserState
    num_temps = 3

    @dataclass
    class Params:
        kit: Any                    # SfxKit
        sample_rate: float
        freq_mul: Any = 1.0         # float, or float32 CUDA tensor [n_voices]
        carrier_mul: Any = 1.0
        modulator_mul: Any = 1.0
        modulator_rad: Any = 1.0
        effect: Any = 0             # int, or int32 CUDA tensor [n_voices]: the index into the kit

    _span_fields = (("freq_mul", "constant"), ("carrier_mul", "constant"), ("modulator_mul", "constant"), ("modulator_rad", "constant"),
                    ("effect", "tag"))

    @staticmethod
    def _cparams(params):
        return abi.LaserParams(params.sample_rate, 0, as_f32(params.freq_mul), as_f32(params.carrier_mul), as_f32(params.modulator_mul),
                               as_f32(params.modulator_rad), as_u32(params.effect), params.kit.handle)

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        self._paint(span, outputs, temps, note_id_changed, self._cparams(params), zero_first)


class Detuned(_Module):
    """examples/example_detuned.zig:31-169: OuterInstrument over Instrument -- a sawtooth whose frequency is warbled by
    low-passed white noise, enveloped, then low-passed again -- as one fused kernel.  outputs = [voice image] or [voice image,
    frequency image] (the reference's oscilloscope sync; None or left out: not painted).  `first_seed`: voice v's noise is
    seeded like the (first_seed + v)-th Noise.init()."""
    _prefix = "detuned"
    _state_ctype = abi.DetunedState
    num_outputs = 2
    num_temps = 4

    @dataclass
    class Patch:                    # the reference's constants (:146, :153, :71, :76, :81-84, :95, :98)
        warble_hz: float = 4.0
        warble_wide: float = 4.0
        color: float = 0.0
        volume: float = 0.75
        attack: float = 0.025       # the three curves are cubed
        decay: float = 0.1
        release: float = 1.0
        sustain_volume: float = 0.5
        cutoff_hz: float = 880.0
        res: float = 0.8

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]
        mode: Any = 0               # int, or int32 CUDA tensor [n_voices]: bit 0 set = narrow warble
        patch: Any = None           # Detuned.Patch; None = the reference's

    _span_fields = (("freq", "constant"), ("note_on", "boolean"), ("mode", "tag"))

    def __init__(self, n_voices, ctx=None, first_seed=0):
        super().__init__(n_voices, ctx, C.c_uint64(first_seed))

    @staticmethod
    def _cparams(params):
        p = params.patch or Detuned.Patch()
        patch = abi.DetunedPatch(p.warble_hz, p.warble_wide, p.color, p.volume, p.attack, p.decay, p.release, p.sustain_volume,
                                 p.cutoff_hz, p.res)
        return abi.DetunedParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on), as_u32(params.mode), patch)

    @staticmethod
    def _outputs(outputs):
        """the C side reads outputs[0] and outputs[1]: a missing frequency image is a zh_buf whose ptr is NULL"""
        outs = list(outputs)
        arr = (abi.Buf * 2)()
        arr[0] = as_buf(outs[0])
        if len(outs) > 1 and outs[1] is not None:
            arr[1] = as_buf(outs[1])
        return arr

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        cp = self._cparams(params)
        rc = self.lib.zh_detuned_paint(self.handle, span.start, span.end, self._outputs(outputs), None, as_bool(note_id_changed), C.byref(cp),
                                       abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, "zh_detuned_paint")

    def _paint_spans(self, span, outputs, temps, params, table, flags, span_params=None):
        cp = self._cparams(params)
        tb, sp = table.device(self.ctx.device, [n for n, _ in self._span_fields])
        if span_params is not None:
            sp = span_params
        rc = self.lib.zh_detuned_paint_spans(self.handle, span.start, span.end, self._outputs(outputs), None, C.byref(cp), sp, C.byref(tb), flags)
        self._keep = (cp, outputs, table)
        return rc


class _Lead(_Module):
    """What the two monophonic leads share: one Params record (sample_rate, freq, note_on, the patch), outputs = [voice image]
    or [voice image, frequency image] (the reference's oscilloscope sync; None or left out: not painted)."""
    num_outputs = 2
    num_temps = 3
    _span_fields = (("freq", "constant"), ("note_on", "boolean"))

    @staticmethod
    def _outputs(outputs):
        """the C side reads outputs[0] and outputs[1]: a missing frequency image is a zh_buf whose ptr is NULL"""
        outs = list(outputs)
        arr = (abi.Buf * 2)()
        arr[0] = as_buf(outs[0])
        if len(outs) > 1 and outs[1] is not None:
            arr[1] = as_buf(outs[1])
        return arr

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False):
        cp = self._cparams(params)
        fn = getattr(self.lib, f"zh_{self._prefix}_paint")
        rc = fn(self.handle, span.start, span.end, self._outputs(outputs), None, as_bool(note_id_changed), C.byref(cp),
                abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, f"zh_{self._prefix}_paint")

    def _paint_spans(self, span, outputs, temps, params, table, flags, span_params=None):
        cp = self._cparams(params)
        tb, sp = table.device(self.ctx.device, [n for n, _ in self._span_fields])
        if span_params is not None:
            sp = span_params
        fn = getattr(self.lib, f"zh_{self._prefix}_paint_spans")
        rc = fn(self.handle, span.start, span.end, self._outputs(outputs), None, C.byref(cp), sp, C.byref(tb), flags)
        self._keep = (cp, outputs, table)
        return rc


class CurveVoice(_Lead):
    """examples/example_curve.zig:33-96: CurvePlayer -- two Curves (modulator frequency, carrier frequency) driving a
    phase-modulated pair of SineOscs, the carrier added straight into the output -- as one fused kernel.  outputs = [voice image]
    or [voice image, frequency image] (the reference's oscilloscope sync; None or left out: not painted).  The curves come from
    an effect kit (zang_amd.sfx.SfxKit; sfx.curve_example_effect() is the reference's pair): the voice plays an effect's
    modulator and carrier curves and never reads its volume curve."""
    _prefix = "curve_player"
    _state_ctype = abi.CurvePlayerState
    num_temps = 2

    @dataclass
    class Params:
        kit: Any                    # SfxKit
        sample_rate: float
        rel_freq: Any = 1.0         # float, or float32 CUDA tensor [n_voices]
        effect: Any = 0             # int, or int32 CUDA tensor [n_voices]: the index into the kit

    _span_fields = (("rel_freq", "constant"), ("effect", "tag"))

    @staticmethod
    def _cparams(params):
        return abi.CurvePlayerParams(params.sample_rate, 0, as_f32(params.rel_freq), as_u32(params.effect), params.kit.handle)


class Porta(_Lead):
    """examples/example_portamento.zig:20-87: a sine whose frequency glides toward the note's (Portamento), scaled by an Envelope,
    as one fused kernel.  The voice carries prev_note_on across sub-spans and buffers: the glide is instantaneous and the
    envelope restarts only when no note was on before."""
    _prefix = "porta"
    _state_ctype = abi.PortaState

    @dataclass
    class Patch:                    # the reference's constants (:57, :68-71)
        glide_curve: int = abi.CURVE_CUBED
        glide: float = 0.5
        attack: float = 0.025       # the three curves are cubed
        decay: float = 0.1
        release: float = 1.0
        sustain_volume: float = 0.5

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]
        patch: Any = None           # Porta.Patch; None = the reference's

    @staticmethod
    def _cparams(params):
        p = params.patch or Porta.Patch()
        patch = abi.PortaPatch(int(p.glide_curve), p.glide, p.attack, p.decay, p.release, p.sustain_volume)
        return abi.PortaParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on), patch)


class Vibrato(_Lead):
    """examples/example_vibrato.zig:17-69: a pulse whose frequency a slow sine modulates, scaled by a Gate, as one fused kernel.
    note_id_changed reaches no module of this voice."""
    _prefix = "vibrato"
    _state_ctype = abi.VibratoState

    @dataclass
    class Patch:                    # the reference's constants (:49, :54, :61)
        vib_hz: float = 4.0
        depth: float = 0.02
        color: float = 0.5

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]
        patch: Any = None           # Vibrato.Patch; None = the reference's

    @staticmethod
    def _cparams(params):
        p = params.patch or Vibrato.Patch()
        return abi.VibratoParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on), abi.VibratoPatch(p.vib_hz, p.depth, p.color))


class HardSquare(_Lead):
    """examples/modules.zig:250-289 HardSquareInstrument: a PulseOsc of color 0.5 times a Gate, as one fused kernel, with the
    frequency image examples/example_arpeggiator.zig:115 adds beside it (outputs[1]; None or left out: not painted).  Inside a
    sub-span every frame is added to, with the gate at 0 too.  note_id_changed reaches no module of this voice."""
    _prefix = "hard_square"
    _state_ctype = abi.HardSquareState
    num_temps = 2

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]

    @staticmethod
    def _cparams(params):
        return abi.HardSquareParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on))


class SawEnv(_Lead):
    """examples/example_subsong.zig:24-68 InnerInstrument: a TriSawOsc of constant frequency times an Envelope whose three curves
    are cubed, as one fused kernel with one output.  Inside a sub-span every frame is added to, where either module paints
    nothing too.  note_id_changed reaches the Envelope."""
    _prefix = "saw_env"
    _state_ctype = abi.SawEnvState
    num_outputs = 1
    num_temps = 2

    @dataclass
    class Patch:                    # the reference's constants (:55, :60-63)
        color: float = 0.0
        attack: float = 0.025       # the three curves are cubed
        decay: float = 0.1
        release: float = 0.15
        sustain_volume: float = 0.5

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]
        patch: Any = None           # SawEnv.Patch; None = the reference's

    @staticmethod
    def _outputs(outputs):
        return (abi.Buf * 1)(as_buf(list(outputs)[0]))

    @staticmethod
    def _cparams(params):
        p = params.patch or SawEnv.Patch()
        patch = abi.SawEnvPatch(p.color, p.attack, p.decay, p.release, p.sustain_volume)
        return abi.SawEnvParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on), patch)


class Dual(_Lead):
    """examples/example_two.zig:109-138, :153: a TriSawOsc of constant frequency and color times an Envelope whose three curves are
    cubed, as one fused kernel, with the frequency image of :109 beside it (outputs[1]; None or left out: not painted).  One voice
    driven by two sources: freq from one, color from the other, note_on and note_id_changed from both (two.SpanMerge).  Inside a
    sub-span every frame is added to, where either module paints nothing too; frames no sub-span covers are left alone (the
    example's whole-buffer multiply turns a -0.0 there into +0.0; with zero_first the two are identical)."""
    _prefix = "dual"
    _state_ctype = abi.DualState
    num_temps = 2
    _span_fields = (("freq", "constant"), ("color", "constant"), ("note_on", "boolean"))

    @dataclass
    class Patch:                    # the reference's constants (:132-135)
        attack: float = 0.025       # the three curves are cubed
        decay: float = 0.1
        release: float = 1.0
        sustain_volume: float = 0.5

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        color: Any = 0.5            # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]
        patch: Any = None           # Dual.Patch; None = the reference's

    @staticmethod
    def _cparams(params):
        p = params.patch or Dual.Patch()
        patch = abi.DualPatch(p.attack, p.decay, p.release, p.sustain_volume)
        return abi.DualParams(params.sample_rate, 0, as_f32(params.freq), as_f32(params.color), as_bool(params.note_on), patch)


class PMCtl(_Module):
    """examples/example_mouse.zig:24-73 over examples/modules.zig:6-77: the phase-modulation instrument whose `relative` is a
    parameter and whose ratio and multiplier are signals, as one fused kernel.  paint() and paint_spans() take the two as
    zang.constant(...) (a float, or per voice) or zang.buffer(image); paint_controlled() is MainModule.paint (:148-211): each of
    the two is a Portamento driven by its own sub-span table (a Control), painted in registers under the voice.  `temps`: None, or
    three entries of which [1] may be a [frame][voice] image the caller keeps between calls -- the reference's stale temp
    (include/zang_hip.h, "ONE DIFFERENCE"): read in the relative / buffer branch, overwritten with the envelope's temp."""
    _prefix = "pmctl"
    _state_ctype = abi.PMCtlState
    num_temps = 3
    _span_fields = (("freq", "constant"), ("note_on", "boolean"))
    _control_fields = (("value", "constant"), ("note_on", "boolean"))

    @dataclass
    class Patch:                    # the reference's constants (:160, :184, :65-68)
        ctl_curve: int = abi.CURVE_LINEAR
        ctl_glide: float = 0.1
        attack: float = 0.025       # the three curves are cubed
        decay: float = 0.1
        release: float = 1.0
        sustain_volume: float = 0.5

    @dataclass
    class Params:
        sample_rate: float
        freq: Any = 220.0           # float, or float32 CUDA tensor [n_voices]
        note_on: Any = True         # bool, or uint8 / bool CUDA tensor [n_voices]
        relative: Any = True        # bool, or uint8 / bool CUDA tensor [n_voices]
        patch: Any = None           # PMCtl.Patch; None = the reference's

    @dataclass
    class Control:
        """one control stream: `table` a span table view with arrays named `value` (f) and `note_on` (u), e.g. a live bank's
        script_table() or control_table(); goal = value * scale (a float, or float32 CUDA tensor [n_voices])"""
        table: Any
        scale: Any = 1.0
        value: str = "value"
        note_on: str = "note_on"

    @staticmethod
    def _cparams(params):
        p = params.patch or PMCtl.Patch()
        patch = abi.PMCtlPatch(int(p.ctl_curve), p.ctl_glide, p.attack, p.decay, p.release, p.sustain_volume)
        return abi.PMCtlParams(params.sample_rate, 0, as_f32(params.freq), as_bool(params.note_on), as_bool(params.relative), patch)

    @classmethod
    def control_table(cls, count, start, end, note_id_changed, value, note_on):
        """a control's sub-span table from host arrays: count [V]; the rest [K][V]"""
        from .script import ScriptSpanTable
        return ScriptSpanTable([(n, k, None) for n, k in cls._control_fields], count, start, end, note_id_changed,
                               {"value": (value, None), "note_on": (None, note_on)})

    @staticmethod
    def _temps(temps):
        if not temps or len(temps) < 2 or temps[1] is None:
            return None
        arr = (abi.Buf * 3)()
        arr[1] = as_buf(temps[1])
        return arr

    def _control(self, ctl):
        tb, sp = ctl.table.device(self.ctx.device, [ctl.value, ctl.note_on])
        c = abi.PMCtlControl(C.pointer(tb), sp[0], sp[1], as_f32(ctl.scale))
        c._keep = (tb, sp, ctl)
        return c

    def _paint_rc(self, span, outputs, temps, note_id_changed, params, ratio, multiplier, flags):
        cp = self._cparams(params)
        rc = self.lib.zh_pmctl_paint(self.handle, span.start, span.end, _bufarray(outputs), self._temps(temps), as_bool(note_id_changed),
                                     C.byref(cp), C.byref(ratio), C.byref(multiplier), flags)
        self._keep = (cp, outputs, temps, ratio, multiplier)
        return rc

    def paint(self, span, outputs, temps, note_id_changed, params, ratio, multiplier, zero_first=False):
        abi.check(self._paint_rc(span, outputs, temps, note_id_changed, params, ratio, multiplier,
                                 abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD), "zh_pmctl_paint")

    def _paint_spans(self, span, outputs, temps, params, table, flags, span_params=None, ratio=None, multiplier=None):
        from . import zang
        cp = self._cparams(params)
        tb, sp = table.device(self.ctx.device, [n for n, _ in self._span_fields])
        if span_params is not None:
            sp = span_params
        ratio = zang.constant(1.0) if ratio is None else ratio
        multiplier = zang.constant(1.0) if multiplier is None else multiplier
        rc = self.lib.zh_pmctl_paint_spans(self.handle, span.start, span.end, _bufarray(outputs), self._temps(temps), C.byref(cp), sp, C.byref(tb),
                                           C.byref(ratio), C.byref(multiplier), flags)
        self._keep = (cp, outputs, temps, table, ratio, multiplier)
        return rc

    def paint_spans(self, span, outputs, temps, params, table, ratio=None, multiplier=None, zero_first=False):
        """the Trigger loop of :193-211 for every voice in one launch; ratio / multiplier: cobs, None = constant 1.0"""
        rc = self._paint_spans(span, outputs, temps, params, table, abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD, None, ratio, multiplier)
        abi.check(rc, "zh_pmctl_paint_spans")

    def _paint_controlled(self, span, outputs, temps, params, table, ratio_ctl, multiplier_ctl, flags, span_params=None):
        cp = self._cparams(params)
        tb, sp = table.device(self.ctx.device, [n for n, _ in self._span_fields])
        if span_params is not None:
            sp = span_params
        rc_, mc_ = self._control(ratio_ctl), self._control(multiplier_ctl)
        rc = self.lib.zh_pmctl_paint_controlled(self.handle, span.start, span.end, _bufarray(outputs), self._temps(temps), C.byref(cp), sp,
                                                C.byref(tb), C.byref(rc_), C.byref(mc_), flags)
        self._keep = (cp, outputs, temps, table, rc_, mc_)
        return rc

    def paint_controlled(self, span, outputs, temps, params, table, ratio_ctl, multiplier_ctl, zero_first=False):
        """MainModule.paint (:148-211) for every voice in ONE launch: `table` the notes' sub-spans, the two Controls' their own"""
        rc = self._paint_controlled(span, outputs, temps, params, table, ratio_ctl, multiplier_ctl,
                                    abi.PAINT_ZERO_FIRST if zero_first else abi.PAINT_ADD)
        abi.check(rc, "zh_pmctl_paint_controlled")
