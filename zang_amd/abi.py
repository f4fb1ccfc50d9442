"""ctypes mirror of include/zang_hip.h (the C ABI of libzang_hip.so).

Loading fails loudly when the library is missing: the product has no CPU path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzang_hip.so")

u32, u64, f32, vp = C.c_uint32, C.c_uint64, C.c_float, C.c_void_p

ZH_OK = 0
ZH_ERR_INVALID, ZH_ERR_UNSUPPORTED, ZH_ERR_NO_DEVICE = -1, -2, -3
ZH_ERR_COMM, ZH_ERR_RCCL_BASE = -4, -100
COMM_ID_BYTES = 128
PAINT_ADD, PAINT_ZERO_FIRST = 0, 1
PAINT_PARAMS_UNCHANGED = 4
PAINT_TOLERANT = 8
FM_SPLIT_OPERATORS = 16
FM_PATCH_VALUES = 22
# the order of parameters[0..21] (examples/example_fmsynth.zig:375-398)
(FM_MOD_FREQ_MUL, FM_MOD_WAVEFORM, FM_MOD_VOLUME, FM_MOD_ATTACK, FM_MOD_DECAY, FM_MOD_SUSTAIN, FM_MOD_RELEASE, FM_MOD_TREMOLO,
 FM_MOD_VIBRATO, FM_MOD_FEEDBACK, FM_CAR_FREQ_MUL, FM_CAR_WAVEFORM, FM_CAR_VOLUME, FM_CAR_ATTACK, FM_CAR_DECAY, FM_CAR_SUSTAIN,
 FM_CAR_RELEASE, FM_CAR_TREMOLO, FM_CAR_VIBRATO, FM_TREMOLO_DEPTH, FM_VIBRATO_DEPTH, FM_ALGORITHM) = range(22)
ZH_CAPTURE_COALESCE = 1
MIX_SEQUENTIAL = 2
AUDIO_SIGNED8, AUDIO_SIGNED16_LSB = 0, 1
COB_CONSTANT, COB_BUFFER = 0, 1
CURVE_INSTANTANEOUS, CURVE_LINEAR, CURVE_SQUARED, CURVE_CUBED = 0, 1, 2, 3
NOISE_WHITE, NOISE_PINK = 0, 1
ENV_IDLE, ENV_ATTACK, ENV_DECAY, ENV_SUSTAIN, ENV_RELEASE = range(5)
FILTER_BYPASS, FILTER_LOW_PASS, FILTER_BAND_PASS, FILTER_HIGH_PASS, FILTER_NOTCH, FILTER_ALL_PASS = range(6)
SAMPLE_U8, SAMPLE_S16_LSB, SAMPLE_S24_LSB, SAMPLE_S32_LSB = range(4)
DISTORTION_OVERDRIVE, DISTORTION_CLIP = 0, 1


class Buf(C.Structure):
    _fields_ = [("ptr", vp), ("voices", u32), ("frames", u32), ("stride", u32), ("reserved", u32)]


class F32(C.Structure):
    _fields_ = [("value", f32), ("reserved", u32), ("per_voice", vp)]


class Bool(C.Structure):
    _fields_ = [("value", u32), ("reserved", u32), ("per_voice", vp)]


class Cob(C.Structure):
    _fields_ = [("tag", u32), ("reserved", u32), ("constant", F32), ("buffer", Buf)]


class Curve(C.Structure):
    _fields_ = [("tag", u32), ("reserved", u32), ("duration", F32)]


class SineOscParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", Cob), ("phase", Cob)]


class SineOscState(C.Structure):
    _fields_ = [("t", f32)]


class PulseOscParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", Cob), ("color", F32)]


class PulseOscState(C.Structure):
    _fields_ = [("cnt", u32)]


TriSawOscParams = PulseOscParams


class TriSawOscState(C.Structure):
    _fields_ = [("cnt", u32), ("t", f32)]


class NoiseParams(C.Structure):
    _fields_ = [("color", u32)]


class NoiseState(C.Structure):
    _fields_ = [("r", u64 * 4), ("b", f32 * 7), ("reserved", u32)]


class EnvelopeParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("attack", Curve), ("decay", Curve), ("release", Curve),
                ("sustain_volume", F32), ("note_on", Bool)]


class EnvelopeState(C.Structure):
    _fields_ = [("state", u32), ("t", f32), ("last_value", f32), ("start", f32)]


class GateParams(C.Structure):
    _fields_ = [("note_on", Bool)]


class FilterParams(C.Structure):
    _fields_ = [("input", Buf), ("type", u32), ("reserved", u32), ("cutoff", Cob), ("res", Cob)]


class FilterState(C.Structure):
    _fields_ = [("l", f32), ("b", f32)]


class Sample(C.Structure):
    _fields_ = [("num_channels", u64), ("sample_rate", u64), ("format", u32), ("reserved", u32),
                ("data", vp), ("data_len", u64)]


class SamplerParams(C.Structure):
    _fields_ = [("sample_rate", F32), ("sample", Sample), ("channel", u64), ("loop", u32), ("reserved", u32)]


class SamplerState(C.Structure):
    _fields_ = [("t", f32)]


class U32(C.Structure):                    # zh_u32
    _fields_ = [("value", u32), ("reserved", u32), ("per_voice", vp)]


class SamplerKitParams(C.Structure):       # zh_sampler_kit_params
    _fields_ = [("sample_rate", F32), ("loop", Bool), ("sample", U32), ("channel", U32), ("kit", vp)]


class DecimatorParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("input", Buf), ("fake_sample_rate", F32)]


class DecimatorState(C.Structure):
    _fields_ = [("dval", f32), ("dcount", f32)]


class DistortionParams(C.Structure):
    _fields_ = [("input", Buf), ("type", u32), ("reserved", u32), ("ingain", F32), ("outgain", F32), ("offset", F32)]


class DelayParams(C.Structure):
    _fields_ = [("input", Buf)]


class FilteredEchoesParams(C.Structure):
    _fields_ = [("input", Buf), ("feedback_volume", F32), ("cutoff", F32)]


class StereoEchoesParams(C.Structure):
    _fields_ = [("input", Buf), ("feedback_volume", F32), ("cutoff", F32)]


class NoiseFilterParams(C.Structure):
    _fields_ = [("color", u32), ("type", u32), ("cutoff", F32), ("res", F32)]


class NoiseFilterState(C.Structure):
    _fields_ = [("noise", NoiseState), ("flt", FilterState)]


class ScriptParam(C.Structure):            # zh_script_param
    _fields_ = [("kind", u32), ("u", u32), ("f", f32), ("is_buffer", u32), ("pf", vp), ("pb", vp), ("stride", u32), ("reserved", u32)]


SP_CONSTANT, SP_BOOLEAN, SP_COB, SP_BUFFER, SP_ENUM, SP_CURVE = range(6)
SCRIPT_MAX_PARAMS = 16


class ScriptSpanTable(C.Structure):        # zh_script_span_table
    _fields_ = [("max_spans", u32), ("reserved", u32), ("count", vp), ("start", vp), ("end", vp), ("note_id_changed", vp)]


class ScriptSpanParam(C.Structure):        # zh_script_span_param
    _fields_ = [("f", vp), ("u", vp)]


ZSCRIPT_FORM_SPANS = 8

# zh_<module>_paint_spans: the index of each span field in span_params (include/zang_hip.h ZH_<MODULE>_SPAN_*), in order
SINEOSC_SPAN_FREQ, SINEOSC_SPAN_PHASE, SINEOSC_SPAN_FIELDS = range(3)
PULSEOSC_SPAN_FREQ, PULSEOSC_SPAN_COLOR, PULSEOSC_SPAN_FIELDS = range(3)
TRISAWOSC_SPAN_FREQ, TRISAWOSC_SPAN_COLOR, TRISAWOSC_SPAN_FIELDS = range(3)
NOISE_SPAN_COLOR, NOISE_SPAN_FIELDS = range(2)
(ENVELOPE_SPAN_ATTACK, ENVELOPE_SPAN_DECAY, ENVELOPE_SPAN_RELEASE, ENVELOPE_SPAN_SUSTAIN_VOLUME, ENVELOPE_SPAN_NOTE_ON,
 ENVELOPE_SPAN_FIELDS) = range(6)
GATE_SPAN_NOTE_ON, GATE_SPAN_FIELDS = range(2)
FILTER_SPAN_TYPE, FILTER_SPAN_CUTOFF, FILTER_SPAN_RES, FILTER_SPAN_FIELDS = range(4)
SAMPLER_SPAN_SAMPLE_RATE, SAMPLER_SPAN_LOOP, SAMPLER_SPAN_FIELDS = range(3)
SAMPLER_KIT_SPAN_SAMPLE_RATE, SAMPLER_KIT_SPAN_LOOP, SAMPLER_KIT_SPAN_SAMPLE, SAMPLER_KIT_SPAN_CHANNEL, SAMPLER_KIT_SPAN_FIELDS = range(5)
DECIMATOR_SPAN_FAKE_SAMPLE_RATE, DECIMATOR_SPAN_FIELDS = range(2)
DISTORTION_SPAN_TYPE, DISTORTION_SPAN_INGAIN, DISTORTION_SPAN_OUTGAIN, DISTORTION_SPAN_OFFSET, DISTORTION_SPAN_FIELDS = range(5)


class CurveNode(C.Structure):
    _fields_ = [("value", f32), ("t", f32)]


class CurveModuleParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("function", u32), ("curve", vp), ("curve_len", u64)]


class CurveModuleState(C.Structure):
    _fields_ = [("t", f32), ("current_song_note", u32), ("current_song_note_offset", C.c_int32), ("next_song_note", u32)]


class CycleParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("speed", Cob)]


class CycleState(C.Structure):
    _fields_ = [("t", f32)]


class PortamentoParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("curve", Curve), ("goal", F32), ("note_on", Bool), ("prev_note_on", Bool)]


class PortamentoState(C.Structure):
    _fields_ = [("t", f32), ("last_value", f32), ("start", f32)]


class NiceParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool)]


class NiceState(C.Structure):
    _fields_ = [("osc", PulseOscState), ("flt", FilterState), ("env", EnvelopeState)]


PMOscParams = NiceParams


class PMOscState(C.Structure):
    _fields_ = [("carrier", SineOscState), ("modulator", SineOscState), ("env", EnvelopeState)]


class FMPatch(C.Structure):
    _fields_ = [("value", u32 * FM_PATCH_VALUES)]


class FMParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("tremolo_input", Buf), ("vibrato_input", Buf), ("freq", F32), ("note_on", Bool)]


class FMOpState(C.Structure):
    _fields_ = [("t", f32), ("feedback1", f32), ("feedback2", f32), ("reserved", u32), ("env", EnvelopeState)]


class FMState(C.Structure):
    _fields_ = [("modulator", FMOpState), ("carrier", FMOpState)]


class SfxCurve(C.Structure):               # zh_sfx_curve
    _fields_ = [("nodes", vp), ("count", u32), ("function", u32)]


class SfxEffect(C.Structure):              # zh_sfx_effect
    _fields_ = [("modulator", SfxCurve), ("carrier", SfxCurve), ("volume", SfxCurve)]


class LaserParams(C.Structure):            # zh_laser_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq_mul", F32), ("carrier_mul", F32), ("modulator_mul", F32),
                ("modulator_rad", F32), ("effect", U32), ("kit", vp)]


class LaserState(C.Structure):             # zh_laser_state: the field order of examples/example_laser.zig:51-55
    _fields_ = [("carrier_curve", CurveModuleState), ("carrier", SineOscState), ("modulator_curve", CurveModuleState),
                ("modulator", SineOscState), ("volume_curve", CurveModuleState)]


LASER_SPAN_FREQ_MUL, LASER_SPAN_CARRIER_MUL, LASER_SPAN_MODULATOR_MUL, LASER_SPAN_MODULATOR_RAD, LASER_SPAN_EFFECT, LASER_SPAN_FIELDS = range(6)


class CurvePlayerParams(C.Structure):      # zh_curve_player_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("rel_freq", F32), ("effect", U32), ("kit", vp)]


class CurvePlayerState(C.Structure):       # zh_curve_player_state: the field order of examples/example_curve.zig:41-44
    _fields_ = [("carrier_curve", CurveModuleState), ("carrier", SineOscState), ("modulator_curve", CurveModuleState),
                ("modulator", SineOscState)]


CURVE_PLAYER_SPAN_REL_FREQ, CURVE_PLAYER_SPAN_EFFECT, CURVE_PLAYER_SPAN_FIELDS = range(3)


class DetunedPatch(C.Structure):           # zh_detuned_patch: the constants of examples/example_detuned.zig
    _fields_ = [("warble_hz", f32), ("warble_wide", f32), ("color", f32), ("volume", f32), ("attack", f32), ("decay", f32),
                ("release", f32), ("sustain_volume", f32), ("cutoff_hz", f32), ("res", f32)]


class DetunedParams(C.Structure):          # zh_detuned_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool), ("mode", U32), ("patch", DetunedPatch)]


class DetunedState(C.Structure):           # zh_detuned_state: the field order of examples/example_detuned.zig:113-115, :41-43
    _fields_ = [("noise", NoiseState), ("noise_filter", FilterState), ("osc", TriSawOscState), ("env", EnvelopeState),
                ("main_filter", FilterState)]


DETUNED_SPAN_FREQ, DETUNED_SPAN_NOTE_ON, DETUNED_SPAN_MODE, DETUNED_SPAN_FIELDS = range(4)


class PortaPatch(C.Structure):             # zh_porta_patch: the constants of examples/example_portamento.zig
    _fields_ = [("glide_curve", u32), ("glide", f32), ("attack", f32), ("decay", f32), ("release", f32), ("sustain_volume", f32)]


class PortaParams(C.Structure):            # zh_porta_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool), ("patch", PortaPatch)]


class PortaState(C.Structure):             # zh_porta_state: the field order of examples/example_portamento.zig:29-32
    _fields_ = [("porta", PortamentoState), ("env", EnvelopeState), ("osc", SineOscState), ("prev_note_on", u32)]


PORTA_SPAN_FREQ, PORTA_SPAN_NOTE_ON, PORTA_SPAN_FIELDS = range(3)


class VibratoPatch(C.Structure):           # zh_vibrato_patch: the constants of examples/example_vibrato.zig
    _fields_ = [("vib_hz", f32), ("depth", f32), ("color", f32)]


class VibratoParams(C.Structure):          # zh_vibrato_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool), ("patch", VibratoPatch)]


class VibratoState(C.Structure):           # zh_vibrato_state: the field order of examples/example_vibrato.zig:26-28
    _fields_ = [("vib", SineOscState), ("osc", PulseOscState)]


VIBRATO_SPAN_FREQ, VIBRATO_SPAN_NOTE_ON, VIBRATO_SPAN_FIELDS = range(3)


class HardSquareParams(C.Structure):       # zh_hard_square_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool)]


class HardSquareState(C.Structure):        # zh_hard_square_state: examples/modules.zig:259-260 (the Gate has no state)
    _fields_ = [("osc", PulseOscState)]


HARD_SQUARE_SPAN_FREQ, HARD_SQUARE_SPAN_NOTE_ON, HARD_SQUARE_SPAN_FIELDS = range(3)


class ArpState(C.Structure):               # zh_arp_state: examples/example_arpeggiator.zig:31-36 without the instrument
    _fields_ = [("next_frame", u64), ("next_id", u64), ("last_note", C.c_int32), ("has_note", u32), ("note_id", u64), ("freq", f32),
                ("note_on", u32)]


ARP_SPAN_FREQ, ARP_SPAN_NOTE_ON, ARP_SPAN_FIELDS = range(3)


class KeyFanState(C.Structure):            # zh_keyfan_state: Voice of examples/example_polyphony.zig:34-40 without the instrument
    _fields_ = [("next_id", u64), ("down", u32), ("has_note", u32), ("note_id", u64), ("freq", f32), ("note_on", u32)]


KEYFAN_SPAN_FREQ, KEYFAN_SPAN_NOTE_ON, KEYFAN_SPAN_FIELDS = range(3)


class GroupDecimation(C.Structure):        # zh_group_decimation
    _fields_ = [("fake_sample_rate", f32), ("bypass", u32)]


class SawEnvPatch(C.Structure):            # zh_saw_env_patch: the constants of examples/example_subsong.zig:55-63
    _fields_ = [("color", f32), ("attack", f32), ("decay", f32), ("release", f32), ("sustain_volume", f32)]


class SawEnvParams(C.Structure):           # zh_saw_env_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool), ("patch", SawEnvPatch)]


class SawEnvState(C.Structure):            # zh_saw_env_state: the field order of examples/example_subsong.zig:33-34
    _fields_ = [("osc", TriSawOscState), ("env", EnvelopeState)]


SAW_ENV_SPAN_FREQ, SAW_ENV_SPAN_NOTE_ON, SAW_ENV_SPAN_FIELDS = range(3)


class MelodyEvent(C.Structure):            # zh_melody_event: SongEvent, src/zang/notes.zig:130-134
    _fields_ = [("t", f32), ("note_on", u32), ("note_id", u64), ("freq", f32), ("reserved", u32)]


class SubsongState(C.Structure):           # zh_subsong_state: examples/example_subsong.zig:100-102 without the instrument
    _fields_ = [("next_song_event", u32), ("t", f32), ("melody", u32), ("has_note", u32), ("note_id", u64), ("freq", f32),
                ("note_on", u32)]


SUBSONG_IN_FREQ, SUBSONG_IN_NOTE_ON, SUBSONG_IN_MELODY, SUBSONG_IN_FIELDS = range(4)
SUBSONG_SPAN_FREQ, SUBSONG_SPAN_NOTE_ON, SUBSONG_SPAN_FIELDS = range(3)
SUBSONG_NO_MELODY = 0xffffffff


class SpanMergeSource(C.Structure):        # zh_span_merge_source: one source of the merge stage (examples/example_two.zig:93-151)
    _fields_ = [("n_fields", u32), ("on_field", u32), ("kinds", C.c_uint8 * 4)]


SPAN_MERGE_MAX_FIELDS = 4
SPAN_MERGE_NOTE_ON, SPAN_MERGE_NIC_A, SPAN_MERGE_NIC_B, SPAN_MERGE_OWN_FIELDS = range(4)   # counted from A's + B's n_fields


class DualPatch(C.Structure):              # zh_dual_patch: the constants of examples/example_two.zig:132-135
    _fields_ = [("attack", f32), ("decay", f32), ("release", f32), ("sustain_volume", f32)]


class DualParams(C.Structure):             # zh_dual_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("color", F32), ("note_on", Bool), ("patch", DualPatch)]


class DualState(C.Structure):              # zh_dual_state: the field order of examples/example_two.zig:36-37
    _fields_ = [("osc", TriSawOscState), ("env", EnvelopeState)]


DUAL_SPAN_FREQ, DUAL_SPAN_COLOR, DUAL_SPAN_NOTE_ON, DUAL_SPAN_FIELDS = range(4)


class PMCtlPatch(C.Structure):             # zh_pmctl_patch: the constants of examples/example_mouse.zig:160, :184, :65-68
    _fields_ = [("ctl_curve", u32), ("ctl_glide", f32), ("attack", f32), ("decay", f32), ("release", f32), ("sustain_volume", f32)]


class PMCtlParams(C.Structure):            # zh_pmctl_params
    _fields_ = [("sample_rate", f32), ("reserved", u32), ("freq", F32), ("note_on", Bool), ("relative", Bool), ("patch", PMCtlPatch)]


class PMCtlState(C.Structure):             # zh_pmctl_state: the two controls' Portamentos, then PMOscInstrument's modules
    _fields_ = [("ratio", PortamentoState), ("multiplier", PortamentoState), ("carrier", SineOscState), ("modulator", SineOscState),
                ("env", EnvelopeState)]


class PMCtlControl(C.Structure):           # zh_pmctl_control: one control stream of zh_pmctl_paint_controlled
    _fields_ = [("table", C.POINTER(ScriptSpanTable)), ("value", ScriptSpanParam), ("note_on", ScriptSpanParam), ("scale", F32)]


PMCTL_SPAN_FREQ, PMCTL_SPAN_NOTE_ON, PMCTL_SPAN_FIELDS = range(3)


class SpanTable(C.Structure):
    _fields_ = [("max_spans", u32), ("reserved", u32), ("count", vp), ("start", vp), ("end", vp), ("freq", vp),
                ("note_on", vp), ("note_id_changed", vp)]


class Impulse(C.Structure):
    _fields_ = [("frame", u64), ("note_id", u64), ("event_id", u64)]


class Iap(C.Structure):
    _fields_ = [("impulses", C.POINTER(Impulse)), ("paramses", vp), ("len", u64)]


class PaintSpan(C.Structure):
    _fields_ = [("start", u64), ("end", u64), ("note_id_changed", u32), ("reserved", u32), ("params", C.c_uint8 * 64)]


class VoiceBankInstrumentState(C.Structure):     # zh_voice_bank_instrument_state
    _fields_ = [("next_event", u64), ("t", f32), ("reserved", u32)]


class VoiceBankVoiceState(C.Structure):          # zh_voice_bank_voice_state
    _fields_ = [("used", u32), ("note_on", u32), ("note_id", u64), ("event_id", u64), ("has_note", u32), ("reserved", u32),
                ("trigger_note_id", u64), ("trigger_event", u64)]


class BankImpulses(C.Structure):                 # zh_bank_impulses
    _fields_ = [("n", u32), ("instrument", vp), ("frame", vp), ("note_id", vp), ("paramses", vp)]


class VoiceBankLiveVoiceState(C.Structure):      # zh_voice_bank_live_voice_state
    _fields_ = [("used", u32), ("note_on", u32), ("note_id", u64), ("event_id", u64), ("has_note", u32), ("reserved", u32),
                ("trigger_note_id", u64), ("carried", u32 * 16)]


class HCob(C.Structure):
    _fields_ = [("tag", u32), ("constant", f32), ("buffer", C.POINTER(f32))]


class HCurve(C.Structure):
    _fields_ = [("tag", u32), ("duration", f32)]


class SineOscHostParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("freq", HCob), ("phase", HCob)]


class PulseOscHostParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("freq", HCob), ("color", f32)]


class NoiseHostParams(C.Structure):
    _fields_ = [("color", u32)]


class EnvelopeHostParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("attack", HCurve), ("decay", HCurve), ("release", HCurve), ("sustain_volume", f32), ("note_on", u32)]


class GateHostParams(C.Structure):
    _fields_ = [("note_on", u32)]


class FilterHostParams(C.Structure):
    _fields_ = [("input", C.POINTER(f32)), ("type", u32), ("cutoff", HCob), ("res", HCob)]


class SamplerHostParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("num_channels", u64), ("sample_rate_in", u64), ("format", u32), ("data", C.POINTER(C.c_uint8)),
                ("data_len", u64), ("channel", u64), ("loop", u32)]


class DecimatorHostParams(C.Structure):
    _fields_ = [("sample_rate", f32), ("input", C.POINTER(f32)), ("fake_sample_rate", f32)]


class DistortionHostParams(C.Structure):
    _fields_ = [("input", C.POINTER(f32)), ("type", u32), ("ingain", f32), ("outgain", f32), ("offset", f32)]


P = C.POINTER
_hpaint = lambda params: [vp, vp, u32, u32, C.POINTER(C.POINTER(f32)), C.POINTER(C.POINTER(f32)), u32, C.POINTER(params)]
_paint = lambda params: [vp, u32, u32, P(Buf), P(Buf), Bool, P(params), u32]
_paint_spans = lambda params: [vp, u32, u32, P(Buf), P(Buf), P(params), P(ScriptSpanParam), P(ScriptSpanTable), u32]

# name -> (restype, argtypes); must list every ZH_API symbol of include/zang_hip.h
SIGNATURES = {
    "zh_create": (C.c_int, [P(vp), C.c_int]),
    "zh_destroy": (C.c_int, [vp]),
    "zh_set_stream": (C.c_int, [vp, vp]),
    "zh_get_stream": (vp, [vp]),
    "zh_sync": (C.c_int, [vp]),
    "zh_error_string": (C.c_char_p, [C.c_int]),
    "zh_version": (C.c_char_p, []),
    "zh_malloc": (C.c_int, [vp, P(vp), C.c_size_t]),
    "zh_free": (C.c_int, [vp, vp]),
    "zh_upload": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "zh_download": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "zh_buf_alloc": (C.c_int, [vp, P(Buf), u32, u32]),
    "zh_buf_free": (C.c_int, [vp, P(Buf)]),
    "zh_buf_upload_voices": (C.c_int, [vp, Buf, vp, u32]),
    "zh_buf_download_voices": (C.c_int, [vp, vp, Buf, u32]),
    "zh_buf_upload_voice": (C.c_int, [vp, Buf, u32, vp, u32]),
    "zh_buf_download_voice": (C.c_int, [vp, vp, Buf, u32, u32]),
    "zh_form_count": (C.c_int, []),
    "zh_form_info": (C.c_int, [C.c_int, P(C.c_char_p), P(C.c_long), P(C.c_long), P(C.c_char_p)]),
    "zh_last_form": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "zh_graph_begin_capture": (C.c_int, [vp]),
    "zh_graph_begin_capture_flags": (C.c_int, [vp, C.c_uint32]),
    "zh_graph_info": (C.c_int, [vp, P(C.c_uint32), P(C.c_uint32), P(C.c_uint32)]),
    "zh_graph_kernels": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "zh_graph_end_capture": (C.c_int, [vp, P(vp)]),
    "zh_graph_launch": (C.c_int, [vp, vp]),
    "zh_graph_destroy": (C.c_int, [vp]),
    "zh_event_create": (C.c_int, [vp, P(vp)]),
    "zh_event_destroy": (C.c_int, [vp]),
    "zh_event_record": (C.c_int, [vp, vp]),
    "zh_event_elapsed_ms": (C.c_int, [vp, vp, P(f32)]),
    "zh_zero": (C.c_int, [vp, u32, u32, Buf]),
    "zh_set": (C.c_int, [vp, u32, u32, Buf, F32]),
    "zh_copy": (C.c_int, [vp, u32, u32, Buf, Buf]),
    "zh_add": (C.c_int, [vp, u32, u32, Buf, Buf, Buf]),
    "zh_add_into": (C.c_int, [vp, u32, u32, Buf, Buf]),
    "zh_add_scalar": (C.c_int, [vp, u32, u32, Buf, Buf, F32]),
    "zh_add_scalar_into": (C.c_int, [vp, u32, u32, Buf, F32]),
    "zh_multiply": (C.c_int, [vp, u32, u32, Buf, Buf, Buf]),
    "zh_multiply_with": (C.c_int, [vp, u32, u32, Buf, Buf]),
    "zh_multiply_scalar": (C.c_int, [vp, u32, u32, Buf, Buf, F32]),
    "zh_multiply_with_scalar": (C.c_int, [vp, u32, u32, Buf, F32]),
    "zh_mixdown_voices": (C.c_int, [vp, u32, u32, vp, Buf, u32]),
    "zh_mixdown_groups": (C.c_int, [vp, u32, u32, vp, C.c_size_t, Buf, u32, u32]),
    "zh_mixdown_groups_pcm": (C.c_int, [vp, u32, u32, vp, C.c_size_t, Buf, u32, vp, C.c_size_t, u32, u32, u32, f32]),
    "zh_ipc_alloc": (C.c_int, [vp, C.c_size_t, P(vp), vp]),
    "zh_ipc_open": (C.c_int, [vp, vp, P(vp)]),
    "zh_ipc_close": (C.c_int, [vp, vp]),
    "zh_sum_slots": (C.c_int, [vp, vp, vp, u32, C.c_size_t, C.c_size_t, u32]),
    "zh_comm_available": (C.c_int, []),
    "zh_comm_library": (C.c_char_p, []),
    "zh_comm_version": (C.c_int, []),
    "zh_comm_last_error": (C.c_char_p, []),
    "zh_comm_unique_id": (C.c_int, [vp]),
    "zh_comm_create": (C.c_int, [vp, u32, u32, vp, P(vp)]),
    "zh_comm_set_timeout": (C.c_int, [C.c_double]),
    "zh_comm_check": (C.c_int, [vp]),
    "zh_comm_abort": (C.c_int, [vp]),
    "zh_comm_destroy": (C.c_int, [vp]),
    "zh_comm_world": (C.c_int, [vp]),
    "zh_comm_rank": (C.c_int, [vp]),
    "zh_allreduce_mix": (C.c_int, [vp, vp, C.c_size_t]),
    "zh_reduce_mix": (C.c_int, [vp, vp, C.c_size_t, u32]),
    "zh_nice_paint_mix_stereo_batch": (C.c_int, [vp, u32, u32, u32, P(vp), P(vp), F32, F32, P(Bool), P(NiceParams), u32]),
    "zh_sineosc_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_sineosc_destroy": (C.c_int, [vp]),
    "zh_sineosc_get_state": (C.c_int, [vp, vp]),
    "zh_sineosc_set_state": (C.c_int, [vp, vp]),
    "zh_sineosc_paint": (C.c_int, _paint(SineOscParams)),
    "zh_pulseosc_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_pulseosc_destroy": (C.c_int, [vp]),
    "zh_pulseosc_get_state": (C.c_int, [vp, vp]),
    "zh_pulseosc_set_state": (C.c_int, [vp, vp]),
    "zh_pulseosc_paint": (C.c_int, _paint(PulseOscParams)),
    "zh_pulseosc_paint_batch": (C.c_int, [vp, u32, u32, P(Buf), u32, P(PulseOscParams), u32]),
    "zh_trisawosc_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_trisawosc_destroy": (C.c_int, [vp]),
    "zh_trisawosc_get_state": (C.c_int, [vp, vp]),
    "zh_trisawosc_set_state": (C.c_int, [vp, vp]),
    "zh_trisawosc_paint": (C.c_int, _paint(TriSawOscParams)),
    "zh_trisawosc_paint_batch": (C.c_int, [vp, u32, u32, P(Buf), u32, P(TriSawOscParams), u32]),
    "zh_noise_create": (C.c_int, [vp, u32, u64, P(vp)]),
    "zh_noise_destroy": (C.c_int, [vp]),
    "zh_noise_get_state": (C.c_int, [vp, vp]),
    "zh_noise_set_state": (C.c_int, [vp, vp]),
    "zh_selftest_noise_jump": (C.c_int, [u64, u32]),
    "zh_noise_paint": (C.c_int, _paint(NoiseParams)),
    "zh_fft_twiddles": (C.c_int, [P(f32), u32]),
    "zh_fft": (C.c_int, [vp, u32, u32, Buf, Buf]),
    "zh_spectrum_plot": (C.c_int, [vp, u32, Buf, Buf]),
    "zh_spectrum_column": (C.c_int, [vp, u32, Buf, vp, C.c_size_t, u32, C.c_int]),
    "zh_envelope_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_envelope_destroy": (C.c_int, [vp]),
    "zh_envelope_get_state": (C.c_int, [vp, vp]),
    "zh_envelope_set_state": (C.c_int, [vp, vp]),
    "zh_envelope_paint": (C.c_int, _paint(EnvelopeParams)),
    "zh_gate_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_gate_destroy": (C.c_int, [vp]),
    "zh_gate_paint": (C.c_int, _paint(GateParams)),
    "zh_filter_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_filter_destroy": (C.c_int, [vp]),
    "zh_filter_get_state": (C.c_int, [vp, vp]),
    "zh_filter_set_state": (C.c_int, [vp, vp]),
    "zh_filter_paint": (C.c_int, _paint(FilterParams)),
    "zh_filter_cutoff_from_frequency": (C.c_int, [vp, u32, vp, vp, f32]),
    "zh_sampler_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_sampler_destroy": (C.c_int, [vp]),
    "zh_sampler_get_state": (C.c_int, [vp, vp]),
    "zh_sampler_set_state": (C.c_int, [vp, vp]),
    "zh_sampler_paint": (C.c_int, _paint(SamplerParams)),
    "zh_sample_kit_create": (C.c_int, [vp, P(Sample), u32, P(vp)]),
    "zh_sample_kit_destroy": (C.c_int, [vp]),
    "zh_sample_kit_count": (C.c_int, [vp, P(u32)]),
    "zh_sample_kit_sample": (C.c_int, [vp, u32, P(Sample)]),
    "zh_sampler_paint_kit_spans": (C.c_int, _paint_spans(SamplerKitParams)),
    "zh_sampler_paint_kit": (C.c_int, _paint(SamplerKitParams)),
    "zh_decimator_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_decimator_destroy": (C.c_int, [vp]),
    "zh_decimator_get_state": (C.c_int, [vp, vp]),
    "zh_decimator_set_state": (C.c_int, [vp, vp]),
    "zh_decimator_paint": (C.c_int, _paint(DecimatorParams)),
    "zh_decimator_paint_groups": (C.c_int, [vp, u32, u32, vp, C.c_size_t, Buf, u32, f32, vp, u32]),
    "zh_distortion_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_distortion_destroy": (C.c_int, [vp]),
    "zh_distortion_paint": (C.c_int, _paint(DistortionParams)),
    "zh_curve_module_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_curve_module_destroy": (C.c_int, [vp]),
    "zh_curve_module_get_state": (C.c_int, [vp, vp]),
    "zh_curve_module_set_state": (C.c_int, [vp, vp]),
    "zh_curve_module_paint": (C.c_int, _paint(CurveModuleParams)),
    "zh_cycle_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_cycle_destroy": (C.c_int, [vp]),
    "zh_cycle_get_state": (C.c_int, [vp, vp]),
    "zh_cycle_set_state": (C.c_int, [vp, vp]),
    "zh_cycle_paint": (C.c_int, _paint(CycleParams)),
    "zh_portamento_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_portamento_destroy": (C.c_int, [vp]),
    "zh_portamento_get_state": (C.c_int, [vp, vp]),
    "zh_portamento_set_state": (C.c_int, [vp, vp]),
    "zh_portamento_paint": (C.c_int, _paint(PortamentoParams)),
    "zh_poly_voice_create": (C.c_int, [u32, u32, u32, u64, vp, vp, vp, P(vp)]),
    "zh_poly_voice_destroy": (C.c_int, [vp]),
    "zh_poly_voice_reset": (C.c_int, [vp]),
    "zh_poly_voice_schedule": (C.c_int, [vp, f32, vp, u32, u32, vp, vp, vp, vp, vp]),
    "zh_voice_bank_create": (C.c_int, [vp, u32, u32, u32, u32, vp, vp, vp, vp, P(vp)]),
    "zh_voice_bank_destroy": (C.c_int, [vp]),
    "zh_voice_bank_reset": (C.c_int, [vp]),
    "zh_voice_bank_reserve": (C.c_int, [vp, u32]),
    "zh_voice_bank_schedule": (C.c_int, [vp, f32, vp, u32, u32]),
    "zh_voice_bank_script_table": (C.c_int, [vp, u32, P(ScriptSpanTable)]),
    "zh_voice_bank_span_param": (C.c_int, [vp, u32, P(ScriptSpanParam)]),
    "zh_voice_bank_span_table": (C.c_int, [vp, u32, u32, P(SpanTable)]),
    "zh_voice_bank_overflows": (C.c_int, [vp, P(u64)]),
    "zh_voice_bank_get_state": (C.c_int, [vp, P(VoiceBankInstrumentState), P(VoiceBankVoiceState)]),
    "zh_voice_bank_set_state": (C.c_int, [vp, P(VoiceBankInstrumentState), P(VoiceBankVoiceState)]),
    "zh_voice_bank_create_live": (C.c_int, [vp, u32, u32, u32, u32, u32, P(vp)]),
    "zh_voice_bank_schedule_live": (C.c_int, [vp, u32, u32, P(BankImpulses)]),
    "zh_voice_bank_live_get_state": (C.c_int, [vp, P(u64), P(VoiceBankLiveVoiceState)]),
    "zh_voice_bank_live_set_state": (C.c_int, [vp, P(u64), P(VoiceBankLiveVoiceState)]),
    "zh_zscript_compile": (C.c_int, [C.c_char_p, C.c_char_p, u32, P(vp), C.c_char_p, C.c_size_t]),
    "zh_zscript_destroy": (C.c_int, [vp]),
    "zh_zscript_free_text": (None, [vp]),
    "zh_zscript_generate_zig": (C.c_int, [vp, P(vp)]),
    "zh_zscript_generate_hip": (C.c_int, [vp, C.c_char_p, C.c_int, P(vp)]),
    "zh_zscript_generate_hip_forms": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_uint32, P(vp)]),
    "zh_zscript_module_count": (u32, [vp]),
    "zh_zscript_module_info": (C.c_int, [vp, u32, C.c_char_p, C.c_size_t, P(u32), P(u32), P(u32), C.c_char_p, C.c_size_t]),
    "zh_zscript_module_param": (C.c_int, [vp, u32, u32, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "zh_zscript_module_num_temps": (C.c_int, [vp, u32, P(u32)]),
    "zh_script_compile": (C.c_int, [C.c_char_p, P(vp), P(C.c_size_t), C.c_char_p, C.c_size_t]),
    "zh_script_free_code": (None, [vp]),
    "zh_script_load": (C.c_int, [vp, C.c_char_p, P(vp), C.c_char_p, C.c_size_t]),
    "zh_script_load_code": (C.c_int, [vp, vp, C.c_size_t, P(vp)]),
    "zh_script_destroy": (C.c_int, [vp]),
    "zh_script_module_create": (C.c_int, [vp, C.c_char_p, u32, u32, u64, P(vp)]),
    "zh_script_module_destroy": (C.c_int, [vp]),
    "zh_script_module_ranges_ok": (C.c_int, [vp]),
    "zh_script_module_get_state": (C.c_int, [vp, vp]),
    "zh_script_module_set_state": (C.c_int, [vp, vp]),
    "zh_script_module_paint": (C.c_int, [vp, u32, u32, P(Buf), Bool, P(ScriptParam), u32, u32]),
    "zh_script_module_paint_spans": (C.c_int, [vp, u32, u32, P(Buf), P(ScriptParam), u32, P(ScriptSpanParam), P(ScriptSpanTable), u32]),
    "zh_nice_create": (C.c_int, [vp, u32, F32, P(vp)]),
    "zh_nice_destroy": (C.c_int, [vp]),
    "zh_nice_get_state": (C.c_int, [vp, vp]),
    "zh_nice_set_state": (C.c_int, [vp, vp]),
    "zh_nice_paint": (C.c_int, _paint(NiceParams)),
    "zh_nice_paint_mix": (C.c_int, [vp, u32, u32, vp, Bool, P(NiceParams), u32]),
    "zh_nice_paint_mix_stereo": (C.c_int, [vp, u32, u32, vp, vp, F32, F32, Bool, P(NiceParams), u32]),
    "zh_delay_create": (C.c_int, [vp, u32, u32, P(vp)]),
    "zh_delay_destroy": (C.c_int, [vp]),
    "zh_delay_reset": (C.c_int, [vp]),
    "zh_delay_get_state": (C.c_int, [vp, vp, vp]),
    "zh_delay_set_state": (C.c_int, [vp, vp, vp]),
    "zh_delay_paint": (C.c_int, _paint(DelayParams)),
    "zh_filtered_echoes_create": (C.c_int, [vp, u32, u32, P(vp)]),
    "zh_filtered_echoes_destroy": (C.c_int, [vp]),
    "zh_filtered_echoes_reset": (C.c_int, [vp]),
    "zh_filtered_echoes_get_state": (C.c_int, [vp, vp, vp, vp]),
    "zh_filtered_echoes_set_state": (C.c_int, [vp, vp, vp, vp]),
    "zh_filtered_echoes_paint": (C.c_int, _paint(FilteredEchoesParams)),
    "zh_stereo_echoes_create": (C.c_int, [vp, u32, u32, P(vp)]),
    "zh_stereo_echoes_destroy": (C.c_int, [vp]),
    "zh_stereo_echoes_reset": (C.c_int, [vp]),
    "zh_stereo_echoes_get_state": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "zh_stereo_echoes_set_state": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "zh_stereo_echoes_paint": (C.c_int, _paint(StereoEchoesParams)),
    "zh_noise_filter_create": (C.c_int, [vp, u32, u64, P(vp)]),
    "zh_noise_filter_destroy": (C.c_int, [vp]),
    "zh_noise_filter_get_state": (C.c_int, [vp, vp]),
    "zh_noise_filter_set_state": (C.c_int, [vp, vp]),
    "zh_noise_filter_paint": (C.c_int, _paint(NoiseFilterParams)),
    "zh_pmosc_create": (C.c_int, [vp, u32, F32, P(vp)]),
    "zh_pmosc_destroy": (C.c_int, [vp]),
    "zh_pmosc_get_state": (C.c_int, [vp, vp]),
    "zh_pmosc_set_state": (C.c_int, [vp, vp]),
    "zh_pmosc_paint": (C.c_int, _paint(PMOscParams)),
    "zh_fm_patch_default": (C.c_int, [P(FMPatch)]),
    "zh_fm_create": (C.c_int, [vp, u32, u32, P(vp)]),
    "zh_fm_destroy": (C.c_int, [vp]),
    "zh_fm_set_patches": (C.c_int, [vp, vp, u32]),
    "zh_fm_get_state": (C.c_int, [vp, vp]),
    "zh_fm_set_state": (C.c_int, [vp, vp]),
    "zh_fm_paint": (C.c_int, _paint(FMParams)),
    "zh_fm_paint_spans": (C.c_int, [vp, u32, u32, P(Buf), P(Buf), f32, Buf, Buf, P(SpanTable), u32]),
    "zh_sfx_effect_default": (C.c_int, [P(SfxEffect), P(CurveNode)]),
    "zh_sfx_kit_create": (C.c_int, [vp, P(SfxEffect), u32, P(vp)]),
    "zh_sfx_kit_destroy": (C.c_int, [vp]),
    "zh_sfx_kit_count": (C.c_int, [vp, P(u32)]),
    "zh_sfx_kit_effect": (C.c_int, [vp, u32, P(SfxEffect)]),
    "zh_laser_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_laser_destroy": (C.c_int, [vp]),
    "zh_laser_get_state": (C.c_int, [vp, vp]),
    "zh_laser_set_state": (C.c_int, [vp, vp]),
    "zh_laser_paint": (C.c_int, _paint(LaserParams)),
    "zh_laser_paint_spans": (C.c_int, _paint_spans(LaserParams)),
    "zh_sfx_effect_curve_example": (C.c_int, [P(SfxEffect), P(CurveNode)]),
    "zh_curve_player_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_curve_player_destroy": (C.c_int, [vp]),
    "zh_curve_player_get_state": (C.c_int, [vp, vp]),
    "zh_curve_player_set_state": (C.c_int, [vp, vp]),
    "zh_curve_player_paint": (C.c_int, _paint(CurvePlayerParams)),
    "zh_curve_player_paint_spans": (C.c_int, _paint_spans(CurvePlayerParams)),
    "zh_detuned_patch_default": (C.c_int, [P(DetunedPatch)]),
    "zh_detuned_create": (C.c_int, [vp, u32, u64, P(vp)]),
    "zh_detuned_destroy": (C.c_int, [vp]),
    "zh_detuned_get_state": (C.c_int, [vp, vp]),
    "zh_detuned_set_state": (C.c_int, [vp, vp]),
    "zh_detuned_paint": (C.c_int, _paint(DetunedParams)),
    "zh_detuned_paint_spans": (C.c_int, _paint_spans(DetunedParams)),
    "zh_porta_patch_default": (C.c_int, [P(PortaPatch)]),
    "zh_porta_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_porta_destroy": (C.c_int, [vp]),
    "zh_porta_get_state": (C.c_int, [vp, vp]),
    "zh_porta_set_state": (C.c_int, [vp, vp]),
    "zh_porta_paint": (C.c_int, _paint(PortaParams)),
    "zh_porta_paint_spans": (C.c_int, _paint_spans(PortaParams)),
    "zh_vibrato_patch_default": (C.c_int, [P(VibratoPatch)]),
    "zh_vibrato_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_vibrato_destroy": (C.c_int, [vp]),
    "zh_vibrato_get_state": (C.c_int, [vp, vp]),
    "zh_vibrato_set_state": (C.c_int, [vp, vp]),
    "zh_vibrato_paint": (C.c_int, _paint(VibratoParams)),
    "zh_vibrato_paint_spans": (C.c_int, _paint_spans(VibratoParams)),
    "zh_hard_square_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_hard_square_destroy": (C.c_int, [vp]),
    "zh_hard_square_get_state": (C.c_int, [vp, vp]),
    "zh_hard_square_set_state": (C.c_int, [vp, vp]),
    "zh_hard_square_paint": (C.c_int, _paint(HardSquareParams)),
    "zh_hard_square_paint_spans": (C.c_int, _paint_spans(HardSquareParams)),
    "zh_arp_create": (C.c_int, [vp, u32, vp, u32, P(vp)]),
    "zh_arp_destroy": (C.c_int, [vp]),
    "zh_arp_reset": (C.c_int, [vp]),
    "zh_arp_reserve": (C.c_int, [vp, u32]),
    "zh_arp_schedule": (C.c_int, [vp, f32, u32, u32, P(ScriptSpanTable), P(ScriptSpanParam)]),
    "zh_arp_script_table": (C.c_int, [vp, u32, P(ScriptSpanTable)]),
    "zh_arp_span_param": (C.c_int, [vp, u32, P(ScriptSpanParam)]),
    "zh_arp_overflows": (C.c_int, [vp, P(u64)]),
    "zh_arp_get_state": (C.c_int, [vp, vp]),
    "zh_arp_set_state": (C.c_int, [vp, vp]),
    "zh_keyfan_create": (C.c_int, [vp, u32, vp, u32, P(vp)]),
    "zh_keyfan_destroy": (C.c_int, [vp]),
    "zh_keyfan_reset": (C.c_int, [vp]),
    "zh_keyfan_reserve": (C.c_int, [vp, u32]),
    "zh_keyfan_schedule": (C.c_int, [vp, u32, u32, P(ScriptSpanTable), P(ScriptSpanParam)]),
    "zh_keyfan_span_table": (C.c_int, [vp, u32, P(SpanTable)]),
    "zh_keyfan_script_table": (C.c_int, [vp, u32, P(ScriptSpanTable)]),
    "zh_keyfan_span_param": (C.c_int, [vp, u32, P(ScriptSpanParam)]),
    "zh_keyfan_overflows": (C.c_int, [vp, P(u64)]),
    "zh_keyfan_get_state": (C.c_int, [vp, vp]),
    "zh_keyfan_set_state": (C.c_int, [vp, vp]),
    "zh_saw_env_patch_default": (C.c_int, [P(SawEnvPatch)]),
    "zh_saw_env_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_saw_env_destroy": (C.c_int, [vp]),
    "zh_saw_env_get_state": (C.c_int, [vp, vp]),
    "zh_saw_env_set_state": (C.c_int, [vp, vp]),
    "zh_saw_env_paint": (C.c_int, _paint(SawEnvParams)),
    "zh_saw_env_paint_spans": (C.c_int, _paint_spans(SawEnvParams)),
    "zh_span_merge_create": (C.c_int, [vp, u32, P(SpanMergeSource), P(SpanMergeSource), P(vp)]),
    "zh_span_merge_destroy": (C.c_int, [vp]),
    "zh_span_merge_reserve": (C.c_int, [vp, u32]),
    "zh_span_merge_schedule": (C.c_int, [vp, u32, u32, P(ScriptSpanTable), P(ScriptSpanParam), P(ScriptSpanTable), P(ScriptSpanParam)]),
    "zh_span_merge_script_table": (C.c_int, [vp, u32, P(ScriptSpanTable)]),
    "zh_span_merge_span_param": (C.c_int, [vp, u32, P(ScriptSpanParam)]),
    "zh_span_merge_overflows": (C.c_int, [vp, P(u64)]),
    "zh_dual_patch_default": (C.c_int, [P(DualPatch)]),
    "zh_dual_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_dual_destroy": (C.c_int, [vp]),
    "zh_dual_get_state": (C.c_int, [vp, vp]),
    "zh_dual_set_state": (C.c_int, [vp, vp]),
    "zh_dual_paint": (C.c_int, _paint(DualParams)),
    "zh_dual_paint_spans": (C.c_int, _paint_spans(DualParams)),
    "zh_pmctl_patch_default": (C.c_int, [P(PMCtlPatch)]),
    "zh_pmctl_create": (C.c_int, [vp, u32, P(vp)]),
    "zh_pmctl_destroy": (C.c_int, [vp]),
    "zh_pmctl_get_state": (C.c_int, [vp, vp]),
    "zh_pmctl_set_state": (C.c_int, [vp, vp]),
    "zh_pmctl_paint": (C.c_int, _paint(PMCtlParams)[:-1] + [P(Cob), P(Cob), u32]),
    "zh_pmctl_paint_spans": (C.c_int, _paint_spans(PMCtlParams)[:-1] + [P(Cob), P(Cob), u32]),
    "zh_pmctl_paint_controlled": (C.c_int, _paint_spans(PMCtlParams)[:-1] + [P(PMCtlControl), P(PMCtlControl), u32]),
    "zh_melody_kit_create": (C.c_int, [vp, vp, u32, vp, u32, P(vp)]),
    "zh_melody_kit_destroy": (C.c_int, [vp]),
    "zh_melody_kit_count": (C.c_int, [vp, P(u32), P(u32)]),
    "zh_subsong_create": (C.c_int, [vp, u32, vp, f32, P(vp)]),
    "zh_subsong_destroy": (C.c_int, [vp]),
    "zh_subsong_reset": (C.c_int, [vp]),
    "zh_subsong_reserve": (C.c_int, [vp, u32]),
    "zh_subsong_schedule": (C.c_int, [vp, f32, u32, u32, P(ScriptSpanTable), P(ScriptSpanParam)]),
    "zh_subsong_script_table": (C.c_int, [vp, u32, P(ScriptSpanTable)]),
    "zh_subsong_span_param": (C.c_int, [vp, u32, P(ScriptSpanParam)]),
    "zh_subsong_overflows": (C.c_int, [vp, P(u64)]),
    "zh_subsong_get_state": (C.c_int, [vp, vp]),
    "zh_subsong_set_state": (C.c_int, [vp, vp]),
    "zh_pow": (C.c_int, [vp, u32, vp, vp, vp]),
    "zh_sin": (C.c_int, [vp, u32, vp, vp]),
    "zh_cos": (C.c_int, [vp, u32, vp, vp]),
    "zh_atan": (C.c_int, [vp, u32, vp, vp]),
    "zh_mix_down": (C.c_int, [vp, vp, vp, u32, u32, u32, u32, f32]),
    "zh_nice_paint_spans": (C.c_int, [vp, u32, u32, P(Buf), P(Buf), f32, P(SpanTable), u32]),
    "zh_pmosc_paint_spans": (C.c_int, [vp, u32, u32, P(Buf), P(Buf), f32, P(SpanTable), u32]),
    "zh_sineosc_paint_spans": (C.c_int, _paint_spans(SineOscParams)),
    "zh_pulseosc_paint_spans": (C.c_int, _paint_spans(PulseOscParams)),
    "zh_trisawosc_paint_spans": (C.c_int, _paint_spans(TriSawOscParams)),
    "zh_noise_paint_spans": (C.c_int, _paint_spans(NoiseParams)),
    "zh_envelope_paint_spans": (C.c_int, _paint_spans(EnvelopeParams)),
    "zh_gate_paint_spans": (C.c_int, _paint_spans(GateParams)),
    "zh_filter_paint_spans": (C.c_int, _paint_spans(FilterParams)),
    "zh_sampler_paint_spans": (C.c_int, _paint_spans(SamplerParams)),
    "zh_decimator_paint_spans": (C.c_int, _paint_spans(DecimatorParams)),
    "zh_distortion_paint_spans": (C.c_int, _paint_spans(DistortionParams)),
    "zh_noise_state_init": (C.c_int, [vp, u64]),
    "zh_decimator_state_init": (C.c_int, [vp]),
    "zh_sineosc_paint_host": (C.c_int, _hpaint(SineOscHostParams)),
    "zh_pulseosc_paint_host": (C.c_int, _hpaint(PulseOscHostParams)),
    "zh_trisawosc_paint_host": (C.c_int, _hpaint(PulseOscHostParams)),
    "zh_noise_paint_host": (C.c_int, _hpaint(NoiseHostParams)),
    "zh_envelope_paint_host": (C.c_int, _hpaint(EnvelopeHostParams)),
    "zh_gate_paint_host": (C.c_int, _hpaint(GateHostParams)),
    "zh_filter_paint_host": (C.c_int, _hpaint(FilterHostParams)),
    "zh_sampler_paint_host": (C.c_int, _hpaint(SamplerHostParams)),
    "zh_decimator_paint_host": (C.c_int, _hpaint(DecimatorHostParams)),
    "zh_distortion_paint_host": (C.c_int, _hpaint(DistortionHostParams)),
    "zh_impulse_queue_create": (C.c_int, [u32, P(vp)]),
    "zh_impulse_queue_destroy": (C.c_int, [vp]),
    "zh_impulse_queue_push": (C.c_int, [vp, u64, u64, vp]),
    "zh_impulse_queue_consume": (C.c_int, [vp, P(Iap)]),
    "zh_note_tracker_create": (C.c_int, [u32, u64, vp, P(f32), P(u64), P(vp)]),
    "zh_note_tracker_destroy": (C.c_int, [vp]),
    "zh_note_tracker_reset": (C.c_int, [vp]),
    "zh_note_tracker_consume": (C.c_int, [vp, f32, u64, u64, P(Iap)]),
    "zh_polyphony_dispatcher_create": (C.c_int, [u32, u32, u32, P(vp)]),
    "zh_polyphony_dispatcher_destroy": (C.c_int, [vp]),
    "zh_polyphony_dispatcher_reset": (C.c_int, [vp]),
    "zh_polyphony_dispatcher_dispatch": (C.c_int, [vp, Iap, P(Iap)]),
    "zh_trigger_create": (C.c_int, [u32, P(vp)]),
    "zh_trigger_destroy": (C.c_int, [vp]),
    "zh_trigger_reset": (C.c_int, [vp]),
    "zh_trigger_counter": (C.c_int, [vp, u64, u64, Iap]),
    "zh_trigger_next": (C.c_int, [vp, P(PaintSpan)]),
}

_lib = None


class ZangHipError(RuntimeError):
    pass


def load(strict=True):
    """Load libzang_hip.so and bind every declared entry point.

    strict=True raises if any symbol of SIGNATURES is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch bundles its own libamdhip64; load it first so that libzang_hip.so binds to the same HIP
    # runtime (two runtimes in one process cannot both see the device).
    import torch  # noqa: F401
    global LIB_PATH
    LIB_PATH = os.environ.get("ZANG_HIP_LIB", LIB_PATH)       # A/B timing of alternative builds of the same library
    if not os.path.exists(LIB_PATH):
        raise ZangHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). zang_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    missing = []
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing and strict:
        raise ZangHipError(f"libzang_hip.so lacks symbols: {missing}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        lib = load(strict=False)
        msg = lib.zh_error_string(rc).decode()
        if rc == ZH_ERR_COMM or rc <= ZH_ERR_RCCL_BASE:
            msg += ": " + lib.zh_comm_last_error().decode()
        raise ZangHipError(f"{what} failed: {rc} ({msg})")
