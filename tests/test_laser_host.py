"""CPU: the sound-effect voice without a device.  The surface -- the header, the ctypes mirror and the Zig binding declare the
entry points and the five-field enum, struct sizes agree with gcc, NULL handles are refused, Laser._paint_spans and
LaserPlayer.push build the right ctypes arguments -- and the yardstick's own check: tests/laser_reference.py on the reference's
triple, and the shared tables reaching every case the GPU tests rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import laser_cases as lc
from tests import laser_reference as lr
from tests.hostprog import flat_header, mirror_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = [
    "ZH_API int zh_sfx_effect_default(zh_sfx_effect *effect, zh_curve_node *nodes );",
    "ZH_API int zh_sfx_kit_create(zh_ctx *ctx, const zh_sfx_effect *effects, uint32_t n, zh_sfx_kit **out);",
    "ZH_API int zh_sfx_kit_destroy(zh_sfx_kit *kit);",
    "ZH_API int zh_sfx_kit_count(const zh_sfx_kit *kit, uint32_t *count_out);",
    "ZH_API int zh_sfx_kit_effect(const zh_sfx_kit *kit, uint32_t i, zh_sfx_effect *out);",
    "ZH_API int zh_laser_create(zh_ctx *ctx, uint32_t n_voices, zh_laser **out);",
    "ZH_API int zh_laser_destroy(zh_laser *m);",
    "ZH_API int zh_laser_get_state(zh_laser *m, zh_laser_state *host);",
    "ZH_API int zh_laser_set_state(zh_laser *m, const zh_laser_state *host);",
    "ZH_API int zh_laser_paint(zh_laser *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "zh_bool note_id_changed, const zh_laser_params *params, uint32_t flags);",
    "ZH_API int zh_laser_paint_spans(zh_laser *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "const zh_laser_params *params, const zh_script_span_param *span_params, const zh_script_span_table *table, uint32_t flags);",
]
FIELDS = ["FREQ_MUL", "CARRIER_MUL", "MODULATOR_MUL", "MODULATOR_RAD", "EFFECT"]


def test_header_declares_the_entry_points_and_the_field_enum():
    text = flat_header()
    for decl in DECLS:
        assert " ".join(decl.split()) in text, decl
    m = re.search(r"enum \{ (ZH_LASER_SPAN_FREQ_MUL = 0.*?) \};", text)
    assert m, "no ZH_LASER_SPAN_* enum"
    names = [x.strip().split(" ")[0] for x in m.group(1).split(",")]
    assert names == ["ZH_LASER_SPAN_" + f for f in FIELDS] + ["ZH_LASER_SPAN_FIELDS"]
    state = re.search(r"typedef struct zh_laser_state \{(.*?)\} zh_laser_state;", text).group(1)
    assert [x.split()[-1] for x in state.split(";") if x.strip()] == ["carrier_curve", "carrier", "modulator_curve", "modulator", "volume_curve"]


def test_ctypes_mirror_and_python_fields_follow_the_header():
    from zang_amd import abi, modules as mod, sfx
    P, vp, u32 = C.POINTER, C.c_void_p, C.c_uint32
    assert abi.SIGNATURES["zh_sfx_effect_default"] == (C.c_int, [P(abi.SfxEffect), P(abi.CurveNode)])
    assert abi.SIGNATURES["zh_sfx_kit_create"] == (C.c_int, [vp, P(abi.SfxEffect), u32, P(vp)])
    assert abi.SIGNATURES["zh_sfx_kit_destroy"] == (C.c_int, [vp])
    assert abi.SIGNATURES["zh_sfx_kit_count"] == (C.c_int, [vp, P(u32)])
    assert abi.SIGNATURES["zh_sfx_kit_effect"] == (C.c_int, [vp, u32, P(abi.SfxEffect)])
    assert abi.SIGNATURES["zh_laser_create"] == (C.c_int, [vp, u32, P(vp)])
    for name in ("zh_laser_get_state", "zh_laser_set_state"):
        assert abi.SIGNATURES[name] == (C.c_int, [vp, vp])
    assert abi.SIGNATURES["zh_laser_paint"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), abi.Bool, P(abi.LaserParams), u32])
    assert abi.SIGNATURES["zh_laser_paint_spans"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), P(abi.LaserParams),
                                                                P(abi.ScriptSpanParam), P(abi.ScriptSpanTable), u32])
    for i, f in enumerate(FIELDS):
        assert getattr(abi, "LASER_SPAN_" + f) == i
    assert abi.LASER_SPAN_FIELDS == 5
    assert [n.upper() for n, _ in mod.Laser._span_fields] == FIELDS
    assert [n for n, _ in abi.LaserState._fields_] == ["carrier_curve", "carrier", "modulator_curve", "modulator", "volume_curve"]
    assert [n for n in sfx.NOTE_PARAMS.names] == [n for n, _ in lr.Note._fields_] and sfx.NOTE_PARAMS.itemsize == C.sizeof(lr.Note)
    lib = abi.load()
    assert lib.zh_laser_paint_spans.argtypes is not None


def test_struct_sizes_match_gcc():
    from zang_amd import abi
    names = {"zh_sfx_curve": abi.SfxCurve, "zh_sfx_effect": abi.SfxEffect, "zh_laser_params": abi.LaserParams, "zh_laser_state": abi.LaserState}
    seen = {n: size for n, (size, _) in mirror_layout(names, offsets=False)[0].items()}
    assert sorted(seen) == sorted(names) and seen["zh_laser_state"] == 56


def test_zig_binding_declares_them():
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    assert "pub extern fn zh_sfx_kit_create(ctx: ?*Ctx, effects: ?[*]const SfxEffect, n: u32, out: *?*SfxKit) c_int;" in zig
    assert "pub extern fn zh_sfx_kit_effect(kit: ?*const SfxKit, i: u32, out: ?*SfxEffect) c_int;" in zig
    assert "pub extern fn zh_sfx_effect_default(effect: ?*SfxEffect, nodes: ?[*]CurveNode) c_int;" in zig
    assert "pub extern fn zh_laser_create(ctx: ?*Ctx, n_voices: u32, out: *?*Laser) c_int;" in zig
    line = re.search(r"pub extern fn zh_laser_paint_spans\((.*?)\) c_int;", zig)
    assert line and "span_params: ?[*]const ScriptSpanParam" in line.group(1) and "params: ?*const LaserParams" in line.group(1)
    assert re.search(r"pub extern fn zh_laser_paint\(.*note_id_changed: Bool, params: \?\*const LaserParams, flags: u32\) c_int;", zig)
    assert "pub const LASER_SPAN_FIELDS: u32 = 5;" in zig and "pub const LASER_SPAN_EFFECT: u32 = 4;" in zig
    assert "pub const LaserParams = extern struct {" in zig and "kit: ?*const SfxKit = null," in zig


def test_null_handles_are_refused():
    from zang_amd import abi
    lib = abi.load()
    e, h, n = abi.SfxEffect(), C.c_void_p(), C.c_uint32()
    nodes = (abi.CurveNode * 9)()
    assert lib.zh_sfx_kit_create(None, C.byref(e), 1, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_sfx_kit_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_sfx_kit_count(None, C.byref(n)) == abi.ZH_ERR_INVALID
    assert lib.zh_sfx_kit_effect(None, 0, C.byref(e)) == abi.ZH_ERR_INVALID
    assert lib.zh_sfx_effect_default(None, nodes) == abi.ZH_ERR_INVALID and lib.zh_sfx_effect_default(C.byref(e), None) == abi.ZH_ERR_INVALID
    assert lib.zh_laser_create(None, 4, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_laser_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_laser_get_state(None, None) == abi.ZH_ERR_INVALID and lib.zh_laser_set_state(None, None) == abi.ZH_ERR_INVALID
    p = abi.LaserParams()
    assert lib.zh_laser_paint(None, 0, 0, None, None, abi.Bool(), C.byref(p), 0) == abi.ZH_ERR_INVALID
    assert lib.zh_laser_paint_spans(None, 0, 0, None, None, C.byref(p), None, None, 0) == abi.ZH_ERR_INVALID


def test_default_effect_is_the_references_triple():
    """zh_sfx_effect_default (no device): example_laser.zig:22-38 restated, all smoothstep, and what zang_amd.sfx holds"""
    from zang_amd import abi, sfx
    e = abi.SfxEffect()
    nodes = (abi.CurveNode * 9)()
    assert abi.load().zh_sfx_effect_default(C.byref(e), nodes) == 0
    got = [(np.float32(nodes[i].t), np.float32(nodes[i].value)) for i in range(9)]
    want = [(np.float32(t), np.float32(v)) for t, v in sfx.DEFAULT_MODULATOR + sfx.DEFAULT_CARRIER + sfx.DEFAULT_VOLUME]
    assert got == want
    base = C.addressof(nodes)
    for i, c in enumerate((e.modulator, e.carrier, e.volume)):
        assert (c.nodes, c.count, c.function) == (base + 24 * i, 3, sfx.smoothstep)
    assert sfx.presets() == {"player_laser": (2.0, 0.5, 0.5), "enemy_laser": (4.0, 0.125, 1.0), "pain": (0.5, 0.125, 1.0), "web": (1.0, 9.0, 1.0)}


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


def test_paint_spans_builds_the_ctypes_arguments_without_a_device():
    """`effect` and `freq_mul` vary per sub-span, the other three come from the params: one zh_laser_paint_spans call with the span
    and flags, the table's arrays, span_params in the C field order."""
    from zang_amd import abi, modules as mod, zang
    m = object.__new__(mod.Laser)
    m.lib, m.handle, m.ctx, m.n_voices = _FakeLib(), C.c_void_p(1234), _FakeCtx(), 4
    V = 4
    eff = np.array([[1, 2, 3, 7], [0, 5, 1, 1]], np.uint32)
    fm = np.full((2, V), 1.125, np.float32)
    table = m.span_table(np.array([1, 2, 0, 1]), np.array([[0, 0, 0, 10], [0, 512, 0, 0]]), np.array([[1024, 512, 0, 20], [0, 1024, 0, 0]]),
                         np.array([[1, 0, 0, 1], [0, 1, 0, 0]]), {"effect": (None, eff), "freq_mul": (fm, None)})
    out = abi.Buf(0x2000, V, 1024, V, 0)
    rc = m._paint_spans(zang.Span(16, 1000), [out], None, m.Params(_FakeKit(), 48000.0, 1.0, 2.0, 0.5, 0.25, 3), table, abi.PAINT_ZERO_FIRST)
    assert rc == 0
    (args,) = m.lib.fns["zh_laser_paint_spans"].calls
    handle, s, e, outs, temps, cp, sp, tb, flags = args
    assert (s, e, flags) == (16, 1000, abi.PAINT_ZERO_FIRST) and temps is None and handle.value == 1234
    assert outs[0].ptr == 0x2000 and outs[0].voices == V
    cp = cp._obj
    assert cp.kit == 0x5150 and cp.effect.value == 3 and cp.sample_rate == 48000.0
    assert (cp.freq_mul.value, cp.carrier_mul.value, cp.modulator_mul.value, cp.modulator_rad.value) == (1.0, 2.0, 0.5, 0.25)
    assert cp.effect.per_voice is None and cp.carrier_mul.per_voice is None
    tb = tb._obj
    assert tb.max_spans == 2
    assert np.ctypeslib.as_array(C.cast(tb.count, C.POINTER(C.c_uint32)), (V,)).tolist() == [1, 2, 0, 1]
    assert np.ctypeslib.as_array(C.cast(tb.note_id_changed, C.POINTER(C.c_uint8)), (2, V)).tolist() == [[1, 0, 0, 1], [0, 1, 0, 0]]
    assert sp[abi.LASER_SPAN_EFFECT].f is None
    assert np.ctypeslib.as_array(C.cast(sp[abi.LASER_SPAN_EFFECT].u, C.POINTER(C.c_uint32)), (2, V)).tolist() == eff.tolist()
    assert sp[abi.LASER_SPAN_FREQ_MUL].u is None
    assert np.ctypeslib.as_array(C.cast(sp[abi.LASER_SPAN_FREQ_MUL].f, C.POINTER(C.c_float)), (2, V)).tolist() == fm.tolist()
    for i in (abi.LASER_SPAN_CARRIER_MUL, abi.LASER_SPAN_MODULATOR_MUL, abi.LASER_SPAN_MODULATOR_RAD):
        assert sp[i].f is None and sp[i].u is None
    with pytest.raises(KeyError):
        m.span_table(np.ones(3), np.zeros((1, 3)), np.full((1, 3), 64), np.zeros((1, 3)), {"cutoff": (np.ones((1, 3)), None)})


def test_player_push_builds_the_note_records_without_a_device():
    """LaserPlayer.push: the four scalars, the effect index and an always-set note_on word per impulse, in push order"""
    from zang_amd import sfx

    class _Bank:
        def __init__(self):
            self.calls = []

        def push(self, *a):
            self.calls.append(a)
    p = object.__new__(sfx.LaserPlayer)
    p.bank = _Bank()
    p.push(2, 17, 5, 3, 1.1, 2.0, 0.5, 0.25)
    p.push([0, 1], [0, 255], [6, 7], [0, 4], [0.9, 1.0], 4.0, 0.125, [1.0, 0.5])
    (a, b) = p.bank.calls
    assert a[:3] == (2, 17, 5) and a[3].dtype == sfx.NOTE_PARAMS and len(a[3]) == 1
    assert a[3][0].tolist() == (np.float32(1.1), 2.0, 0.5, 0.25, 3, 1)
    assert b[3]["effect"].tolist() == [0, 4] and b[3]["note_on"].tolist() == [1, 1] and b[3]["carrier_mul"].tolist() == [4.0, 4.0]
    assert b[3]["modulator_rad"].tolist() == [1.0, 0.5] and b[3]["freq_mul"].tolist() == [np.float32(0.9), 1.0]


# ------------------------------------------------------------------ the yardstick's own check
def test_reference_on_the_default_effect(oracle):
    """one voice, 48 kHz, one impulse at frame 0, a zeroed image: out[0] is +0.0 (the volume curve starts at 0), frames from 9600
    (0.2 s) on hold only +/-0.0, and some frame between is non-zero"""
    kit = lr.Kit(lc.default_kit_effects())
    voice = lr.Voice(oracle)
    F = 12288
    out = np.zeros(F, np.float32)
    temps = [np.zeros(F, np.float32) for _ in range(3)]
    for b in range(F // 1024):
        lr.laser_paint(oracle, voice, kit, b * 1024, (b + 1) * 1024, out, temps, b == 0, 48000.0, 1.0, 2.0, 0.5, 0.5, 0)
    assert out.view(np.uint32)[0] == 0
    assert not (out.view(np.uint32)[9600:] & 0x7FFFFFFF).any()
    assert np.abs(out[1:9600]).max() > 0.5
    # an effect index equal to the count: nothing at all, note_id_changed or not
    before, words = out.copy(), voice.words()
    lr.laser_paint(oracle, voice, kit, 0, 1024, out, temps, True, 48000.0, 1.0, 2.0, 0.5, 0.5, 1)
    assert lc.same_bits(out, before) and voice.words() == words


def test_the_test_tables_reach_every_case_the_issue_names():
    effects = lc.kit_effects()
    assert len(effects) == 5
    assert any(len({fn for _, fn in e}) == 2 for e in effects)                   # linear and smoothstep mixed in one effect
    assert any(len(e[2][0]) == 0 for e in effects)                               # an empty volume curve
    assert any(all(len(c) == 1 for c, _ in e) for e in effects)                  # single nodes
    dense = [c for e in effects for c, _ in e if len(c) > 32]
    assert dense and all(round(c[33][0] * lc.SR) < 144 for c in dense)           # more than 32 nodes inside one sub-span (v0's third)
    tb = lc.tables(130, 130000)
    live = np.arange(lc.MAX_SPANS)[:, None] < tb["count"][None, :]
    assert set(tb["effect"][live].tolist()) == set(range(6))
    assert (live & (tb["effect"] == 5) & (tb["nic"] == 1)).any()                 # the count as an index, note_id_changed set
    assert (live & (tb["start"] == tb["end"])).any() and set(tb["count"].tolist()) == {0, 1, 2, 3, 4}
    assert tb["count"][4] == 0 and tb["start"][1, 1] < tb["end"][0, 1]           # no sub-span; the out-of-order one
    assert tb["nic"][2, 0] == 0 and tb["effect"][2, 0] != tb["effect"][0, 0] and tb["end"][0, 0] - tb["start"][0, 0] == 48
    second = lc.tables(130, 130001, second=True)
    assert not second["nic"][0].any()
    for v in range(130):                                                         # another effect than the voice's last, note_id_changed clear
        if tb["count"][v]:
            assert second["effect"][0, v] != tb["effect"][tb["count"][v] - 1, v]
    base = lc.base_image(8, 1)
    assert (base.view(np.uint32) == 0x80000000).sum() > 100
