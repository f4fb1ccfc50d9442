"""CPU: sample kits without a device.  zang_amd/csrc/sample_kit.hip.h -- the lane k_sampler_kit_spans runs per voice and the
packing functions zh_sample_kit_create calls -- is compiled for the host with AddressSanitizer + UBSan
(tests/cpp/sample_kit_lane_host.cpp: its own main, the blob a heap block of exactly the library's size) and held against
zo_sampler_paint per voice and sub-span, on bits.  Then the surface: the header, the ctypes mirror and the Zig binding declare
the entry points and the four-field enum, struct sizes agree with gcc, read_wav round-trips, NULL handles are refused and
Sampler._paint_kit_spans builds the right call."""
import ctypes as C
import os
import re
import wave

import numpy as np
import pytest

from tests import sample_kit_cases as sk
from tests.hostprog import build_sanitized, flat_header, mirror_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sample_kit_lane_host.cpp")
HEADER = os.path.join(ROOT, "include", "zang_hip.h")

DECLS = [
    "ZH_API int zh_sample_kit_create(zh_ctx *ctx, const zh_sample *samples, uint32_t n, zh_sample_kit **out);",
    "ZH_API int zh_sample_kit_destroy(zh_sample_kit *kit);",
    "ZH_API int zh_sample_kit_count(const zh_sample_kit *kit, uint32_t *count_out);",
    "ZH_API int zh_sample_kit_sample(const zh_sample_kit *kit, uint32_t i, zh_sample *out);",
    "ZH_API int zh_sampler_paint_kit_spans(zh_sampler *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "const zh_sampler_kit_params *params, const zh_script_span_param *span_params, const zh_script_span_table *table, uint32_t flags);",
    "ZH_API int zh_sampler_paint_kit(zh_sampler *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "zh_bool note_id_changed, const zh_sampler_kit_params *params, uint32_t flags);",
]
FIELDS = ["SAMPLE_RATE", "LOOP", "SAMPLE", "CHANNEL"]


# ------------------------------------------------------------------ the lane under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("sample_kit_lane"))


@pytest.mark.parametrize("V", [1, 65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_lane_equals_the_oracle_over_two_carried_buffers(harness, oracle, tmp_path, V, zero_first):
    """Every sub-span of every voice with its own sample, channel, rate and loop flag: the image (rows outside the span and
    frames no sub-span covers included) and `t`, after each of two buffers with carried state.  No sanitizer report: the last
    kit entry is s24 with stray bytes, at the blob's end."""
    samples = sk.kit_samples()
    rng = np.random.default_rng(77 + V)
    t_ref = sk.start_t(V, 5 + V)
    t_got = t_ref.copy()
    for b in range(2):
        tb = sk.tables(V, 1000 * V + b, second=b == 1)
        base = rng.uniform(-1.0, 1.0, (V, sk.ROWS)).astype(np.float32)
        ref, t_ref = sk.reference(oracle, samples, tb, t_ref, base.copy(), zero_first)
        got, t_got = sk.run_lane_harness(harness, str(tmp_path), samples, tb, t_got, base.copy(), zero_first)
        assert sk.same_bits(got, ref), (V, b, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:5])
        assert sk.same_bits(t_got, t_ref), (V, b, t_got, t_ref)
    assert not sk.same_bits(ref, base)                                # something was painted


def test_the_test_tables_reach_every_case_the_issue_names():
    tb = sk.tables(130, 130000)
    samples = sk.kit_samples()
    live = np.arange(sk.MAX_SPANS)[:, None] < tb["count"][None, :]
    assert set(tb["sample"][live].tolist()) == set(range(8))           # every format, the empty sample, the out-of-range index
    nch = np.array([s[0] for s in samples] + [0])[tb["sample"]]
    for nic in (0, 1):
        assert (live & (tb["channel"] >= nch) & (tb["sample"] < 7) & (tb["nic"] == nic)).any()   # channel >= num_channels, both ways
    for loop in (0, 1):
        assert (live & (tb["sample_rate"] < 0) & (tb["loop"] == loop)).any()                      # backwards with and without loop
    assert (live & (tb["start"] == tb["end"])).any() and set(tb["count"].tolist()) == {0, 1, 2, 3, 4}
    assert tb["start"][1, 1] < tb["end"][0, 1]                         # the out-of-order sub-span
    second = sk.tables(130, 130001, second=True)
    assert not second["nic"][0].any()
    for v in range(130):                                               # another sample than the voice's last, note_id_changed clear
        if tb["count"][v]:
            assert second["sample"][0, v] != tb["sample"][tb["count"][v] - 1, v]


# ------------------------------------------------------------------ header, mirror, binding
def test_header_declares_the_entry_points_and_the_field_enum():
    text = flat_header()
    for decl in DECLS:
        assert " ".join(decl.split()) in text, decl
    m = re.search(r"enum \{ (ZH_SAMPLER_KIT_SPAN_SAMPLE_RATE = 0.*?) \};", text)
    assert m, "no ZH_SAMPLER_KIT_SPAN_* enum"
    names = [x.strip().split(" ")[0] for x in m.group(1).split(",")]
    assert names == ["ZH_SAMPLER_KIT_SPAN_" + f for f in FIELDS] + ["ZH_SAMPLER_KIT_SPAN_FIELDS"]
    assert "DEVICE pointer" in open(HEADER).read() and "HOST pointer" in open(HEADER).read()


def test_ctypes_mirror_and_python_fields_follow_the_header():
    from zang_amd import abi, modules as mod
    P, vp, u32 = C.POINTER, C.c_void_p, C.c_uint32
    assert abi.SIGNATURES["zh_sample_kit_create"] == (C.c_int, [vp, P(abi.Sample), u32, P(vp)])
    assert abi.SIGNATURES["zh_sample_kit_destroy"] == (C.c_int, [vp])
    assert abi.SIGNATURES["zh_sample_kit_count"] == (C.c_int, [vp, P(u32)])
    assert abi.SIGNATURES["zh_sample_kit_sample"] == (C.c_int, [vp, u32, P(abi.Sample)])
    assert abi.SIGNATURES["zh_sampler_paint_kit_spans"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), P(abi.SamplerKitParams),
                                                                      P(abi.ScriptSpanParam), P(abi.ScriptSpanTable), u32])
    assert abi.SIGNATURES["zh_sampler_paint_kit"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), abi.Bool, P(abi.SamplerKitParams), u32])
    for i, f in enumerate(FIELDS):
        assert getattr(abi, "SAMPLER_KIT_SPAN_" + f) == i
    assert abi.SAMPLER_KIT_SPAN_FIELDS == 4
    assert [n.upper() for n, _ in mod.Sampler._kit_span_fields] == FIELDS
    assert [n.upper() for n, _ in mod.Sampler._span_fields] == FIELDS[:2]      # the plain span paint keeps its two
    lib = abi.load()
    assert lib.zh_sampler_paint_kit_spans.argtypes is not None


def test_struct_sizes_match_gcc():
    from zang_amd import abi
    names = {"zh_u32": abi.U32, "zh_sampler_kit_params": abi.SamplerKitParams, "zh_sample": abi.Sample}
    seen = {n: size for n, (size, _) in mirror_layout(names, offsets=False)[0].items()}
    assert sorted(seen) == sorted(names)


def test_zig_binding_declares_them():
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    assert "pub extern fn zh_sample_kit_create(ctx: ?*Ctx, samples: ?[*]const Sample, n: u32, out: *?*SampleKit) c_int;" in zig
    assert "pub extern fn zh_sample_kit_sample(kit: ?*const SampleKit, i: u32, out: ?*Sample) c_int;" in zig
    assert "pub extern fn zh_sample_kit_count(kit: ?*const SampleKit, count_out: ?*u32) c_int;" in zig
    line = re.search(r"pub extern fn zh_sampler_paint_kit_spans\((.*?)\) c_int;", zig)
    assert line and "span_params: ?[*]const ScriptSpanParam" in line.group(1) and "params: ?*const SamplerKitParams" in line.group(1)
    assert "table: ?*const ScriptSpanTable" in line.group(1)
    assert re.search(r"pub extern fn zh_sampler_paint_kit\(.*note_id_changed: Bool, params: \?\*const SamplerKitParams, flags: u32\) c_int;", zig)
    assert "pub const SAMPLER_KIT_SPAN_FIELDS: u32 = 4;" in zig and "pub const SAMPLER_SPAN_FIELDS: u32 = 2;" in zig
    assert "pub const SamplerKitParams = extern struct {" in zig and "kit: ?*const SampleKit = null," in zig


# ------------------------------------------------------------------ read_wav
@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("channels", [1, 2])
def test_read_wav_round_trips(tmp_path, width, channels):
    from zang_amd import samplekit
    data = np.random.default_rng(width * 10 + channels).integers(0, 256, 53 * channels * width, dtype=np.uint8).tobytes()
    path = str(tmp_path / "s.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(22050 * width)
        w.writeframes(data)
    assert samplekit.read_wav(path) == (channels, 22050 * width, width - 1, data)


# ------------------------------------------------------------------ refusals that need no device; the call Python builds
def test_null_handles_are_refused():
    from zang_amd import abi
    lib = abi.load()
    s = abi.Sample(1, 44100, 1, 0, None, 0)
    h, n = C.c_void_p(), C.c_uint32()
    assert lib.zh_sample_kit_create(None, C.byref(s), 1, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_sample_kit_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_sample_kit_count(None, C.byref(n)) == abi.ZH_ERR_INVALID
    assert lib.zh_sample_kit_sample(None, 0, C.byref(s)) == abi.ZH_ERR_INVALID
    p = abi.SamplerKitParams()
    assert lib.zh_sampler_paint_kit(None, 0, 0, None, None, abi.Bool(), C.byref(p), 0) == abi.ZH_ERR_INVALID
    assert lib.zh_sampler_paint_kit_spans(None, 0, 0, None, None, C.byref(p), None, None, 0) == abi.ZH_ERR_INVALID


class _FakeFn:
    def __init__(self):
        self.calls = []

    def __call__(self, *args):
        self.calls.append(args)
        return 0


class _FakeLib:
    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        return self.fns.setdefault(name, _FakeFn())


class _FakeCtx:
    device = "cpu"


class _FakeKit:
    handle = C.c_void_p(0x5150)


def test_paint_kit_spans_builds_the_ctypes_arguments_without_a_device():
    """`sample` and `sample_rate` vary per sub-span, `loop` and `channel` come from the params: one zh_sampler_paint_kit_spans
    call with the span and flags, the table's arrays, span_params in the C field order."""
    from zang_amd import abi, modules as mod, zang
    m = object.__new__(mod.Sampler)
    m.lib, m.handle, m.ctx, m.n_voices = _FakeLib(), C.c_void_p(1234), _FakeCtx(), 4
    V = 4
    smp = np.array([[1, 2, 3, 7], [0, 5, 1, 1]], np.uint32)
    rate = np.full((2, V), 22050.0, np.float32)
    table = m.kit_span_table(np.array([1, 2, 0, 1]), np.array([[0, 0, 0, 10], [0, 512, 0, 0]]), np.array([[1024, 512, 0, 20], [0, 1024, 0, 0]]),
                             np.array([[1, 0, 0, 1], [0, 1, 0, 0]]), {"sample": (None, smp), "sample_rate": (rate, None)})
    out = abi.Buf(0x2000, V, 1024, V, 0)
    rc = m._paint_kit_spans(zang.Span(16, 1000), [out], None, m.KitParams(_FakeKit(), 48000.0, 3, 1, True), table, abi.PAINT_ZERO_FIRST)
    assert rc == 0
    (args,) = m.lib.fns["zh_sampler_paint_kit_spans"].calls
    handle, s, e, outs, temps, cp, sp, tb, flags = args
    assert (s, e, flags) == (16, 1000, abi.PAINT_ZERO_FIRST) and temps is None and handle.value == 1234
    assert outs[0].ptr == 0x2000 and outs[0].voices == V
    cp = cp._obj
    assert cp.kit == 0x5150 and cp.sample.value == 3 and cp.channel.value == 1 and cp.loop.value == 1 and cp.sample_rate.value == 48000.0
    assert cp.sample.per_voice is None and cp.sample_rate.per_voice is None
    tb = tb._obj
    assert tb.max_spans == 2
    assert np.ctypeslib.as_array(C.cast(tb.count, C.POINTER(C.c_uint32)), (V,)).tolist() == [1, 2, 0, 1]
    assert np.ctypeslib.as_array(C.cast(tb.note_id_changed, C.POINTER(C.c_uint8)), (2, V)).tolist() == [[1, 0, 0, 1], [0, 1, 0, 0]]
    assert sp[abi.SAMPLER_KIT_SPAN_SAMPLE].f is None
    assert np.ctypeslib.as_array(C.cast(sp[abi.SAMPLER_KIT_SPAN_SAMPLE].u, C.POINTER(C.c_uint32)), (2, V)).tolist() == smp.tolist()
    assert sp[abi.SAMPLER_KIT_SPAN_SAMPLE_RATE].u is None
    assert np.ctypeslib.as_array(C.cast(sp[abi.SAMPLER_KIT_SPAN_SAMPLE_RATE].f, C.POINTER(C.c_float)), (2, V)).tolist() == rate.tolist()
    for i in (abi.SAMPLER_KIT_SPAN_LOOP, abi.SAMPLER_KIT_SPAN_CHANNEL):
        assert sp[i].f is None and sp[i].u is None
    with pytest.raises(KeyError):
        m.kit_span_table(np.ones(3), np.zeros((1, 3)), np.full((1, 3), 64), np.zeros((1, 3)), {"cutoff": (np.ones((1, 3)), None)})


# ------------------------------------------------------------------ hostile rates and play positions
# The rate reaches an address: ratio = sample.sample_rate / rate steps the play position t, and floor(t) / round(t) index the PCM.
# Why no f32 rate or position can take a load outside the sample (csrc/voices.hip.h, csrc/modules.hip k_sampler, csrc/sample_kit.hip.h):
#   * the position becomes an index only through zf32_to_i32, which saturates at +-2^31 and takes NaN to 0; t0 + n and i0 + 1 are
#     formed in uint32, so they wrap instead of overflowing;
#   * every PCM load goes through sampler_at, whose address is (0 <= index < num_samples ? index : 0) * num_channels + channel with
#     channel < num_channels checked on the host, or through the paired load of k_sampler, whose frame is min(max(r0, 0), n - 2) with
#     n >= 2 required for that path; an index outside the sample selects the value 0 AFTER a load from frame 0;
#   * a looped index goes through sampler_mod first, whose result is corrected into [0, n) -- and sampler_at tests it again;
#   * a sample without frames is the format kSampleEmpty, which loads nothing;
#   * every loop runs over the span's frames; none is bounded by t or the ratio.
# Here the lane runs them under ASan / UBSan against the oracle.
HOSTILE_RATES = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 1e-30, 3e38, -3e38, -1.0, 1.0, 2.0, 1e9, 4.3e9,
                 44100.0 / 0.9999, 44100.0 / 1.0001, 44095.59, 44104.41]
HOSTILE_T = [np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, 1e-45, -0.0, -0.5, 4.3e9]


def _same_f32(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_lane_with_hostile_rates_and_positions_equals_the_oracle(harness, oracle, tmp_path, zero_first):
    """Every hostile rate in a sub-span of every kit sample, looped and not, from ordinary and hostile play positions, over two
    carried buffers: no sanitizer report, NaN positions equal, every other sample and `t` bit for bit."""
    samples = sk.kit_samples()
    V = 8 * len(HOSTILE_RATES)
    rng = np.random.default_rng(77)
    t_ref = sk.start_t(V, 5)
    t_ref[4:4 + len(HOSTILE_T)] = HOSTILE_T
    t_got = t_ref.copy()
    painted = 0
    for b in range(2):
        tb = sk.tables(V, 900 + b, second=b == 1)
        v = np.arange(V)
        for k in range(sk.MAX_SPANS):
            hit = (v + k) % 2 == 0                                   # every other sub-span of a voice keeps its ordinary rate
            tb["sample_rate"][k, hit] = np.array(HOSTILE_RATES, np.float32)[(v[hit] // 8 + k) % len(HOSTILE_RATES)]
        base = rng.uniform(-1.0, 1.0, (V, sk.ROWS)).astype(np.float32)
        ref, t_ref = sk.reference(oracle, samples, tb, t_ref, base.copy(), zero_first)
        got, t_got = sk.run_lane_harness(harness, str(tmp_path), samples, tb, t_got, base.copy(), zero_first)
        assert _same_f32(got, ref), (b, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:5])
        assert _same_f32(t_got, t_ref), (b, t_got, t_ref)
        painted += int((ref != base).sum())
        assert np.isnan(ref).mean() <= 0.5
    assert painted > 0
