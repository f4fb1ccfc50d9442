"""CPU: the curve voice without a device.  The surface -- the header, the ctypes mirror and the Zig binding declare the seven
entry points and the two-field enum, struct sizes agree with gcc, NULL handles are refused, the example's effect is the
reference's pair -- and the yardstick's own check: tests/curve_player_reference.py on the example's curves, and the shared tables
reaching every case the GPU tests rely on."""
import ctypes as C
import os
import re

import numpy as np

from tests import curve_player_cases as cc
from tests import curve_player_reference as cr
from tests.hostprog import flat_header, mirror_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zang_amd", "csrc")

DECLS = [
    "ZH_API int zh_sfx_effect_curve_example(zh_sfx_effect *effect, zh_curve_node *nodes );",
    "ZH_API int zh_curve_player_create(zh_ctx *ctx, uint32_t n_voices, zh_curve_player **out);",
    "ZH_API int zh_curve_player_destroy(zh_curve_player *m);",
    "ZH_API int zh_curve_player_get_state(zh_curve_player *m, zh_curve_player_state *host);",
    "ZH_API int zh_curve_player_set_state(zh_curve_player *m, const zh_curve_player_state *host);",
    "ZH_API int zh_curve_player_paint(zh_curve_player *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "zh_bool note_id_changed, const zh_curve_player_params *params, uint32_t flags);",
    "ZH_API int zh_curve_player_paint_spans(zh_curve_player *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "const zh_curve_player_params *params, const zh_script_span_param *span_params, const zh_script_span_table *table, uint32_t flags);",
]
FIELDS = ["REL_FREQ", "EFFECT"]
MEMBERS = ["carrier_curve", "carrier", "modulator_curve", "modulator"]


def test_header_declares_the_entry_points_and_the_field_enum():
    text = flat_header()
    for decl in DECLS:
        assert " ".join(decl.split()) in text, decl
    m = re.search(r"enum \{ (ZH_CURVE_PLAYER_SPAN_REL_FREQ = 0.*?) \};", text)
    assert m, "no ZH_CURVE_PLAYER_SPAN_* enum"
    names = [x.strip().split(" ")[0] for x in m.group(1).split(",")]
    assert names == ["ZH_CURVE_PLAYER_SPAN_" + f for f in FIELDS] + ["ZH_CURVE_PLAYER_SPAN_FIELDS"]
    state = re.search(r"typedef struct zh_curve_player_state \{(.*?)\} zh_curve_player_state;", text).group(1)
    assert [x.split()[-1] for x in state.split(";") if x.strip()] == MEMBERS
    params = re.search(r"typedef struct zh_curve_player_params \{(.*?)\} zh_curve_player_params;", text).group(1)
    assert [x.replace("*", " ").split()[-1] for x in params.split(";") if x.strip()] == ["sample_rate", "reserved", "rel_freq", "effect", "kit"]


def test_ctypes_mirror_and_python_fields_follow_the_header():
    from zang_amd import abi, modules as mod, sfx
    P, vp, u32 = C.POINTER, C.c_void_p, C.c_uint32
    assert abi.SIGNATURES["zh_sfx_effect_curve_example"] == (C.c_int, [P(abi.SfxEffect), P(abi.CurveNode)])
    assert abi.SIGNATURES["zh_curve_player_create"] == (C.c_int, [vp, u32, P(vp)])
    assert abi.SIGNATURES["zh_curve_player_destroy"] == (C.c_int, [vp])
    for name in ("zh_curve_player_get_state", "zh_curve_player_set_state"):
        assert abi.SIGNATURES[name] == (C.c_int, [vp, vp])
    assert abi.SIGNATURES["zh_curve_player_paint"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), abi.Bool, P(abi.CurvePlayerParams), u32])
    assert abi.SIGNATURES["zh_curve_player_paint_spans"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), P(abi.CurvePlayerParams),
                                                                       P(abi.ScriptSpanParam), P(abi.ScriptSpanTable), u32])
    for i, f in enumerate(FIELDS):
        assert getattr(abi, "CURVE_PLAYER_SPAN_" + f) == i
    assert abi.CURVE_PLAYER_SPAN_FIELDS == 2
    assert mod.CurveVoice._span_fields == (("rel_freq", "constant"), ("effect", "tag"))
    assert [n.upper() for n, _ in mod.CurveVoice._span_fields] == FIELDS and issubclass(mod.CurveVoice, mod._Module)
    assert [n for n, _ in abi.CurvePlayerState._fields_] == MEMBERS
    assert [n for n, _ in abi.CurvePlayerParams._fields_] == ["sample_rate", "reserved", "rel_freq", "effect", "kit"]
    assert list(sfx.CURVE_NOTE_PARAMS.names) == [n for n, _ in cr.Note._fields_] and sfx.CURVE_NOTE_PARAMS.itemsize == C.sizeof(cr.Note)
    lib = abi.load()
    assert lib.zh_curve_player_paint_spans.argtypes is not None


def test_struct_sizes_match_gcc():
    from zang_amd import abi
    names = {"zh_curve_player_params": abi.CurvePlayerParams, "zh_curve_player_state": abi.CurvePlayerState}
    seen = {n: size for n, (size, _) in mirror_layout(names, offsets=False)[0].items()}
    assert sorted(seen) == sorted(names) and seen["zh_curve_player_state"] == 40            # ten words per voice


def test_zig_binding_declares_them():
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    assert "pub extern fn zh_sfx_effect_curve_example(effect: ?*SfxEffect, nodes: ?[*]CurveNode) c_int;" in zig
    assert "pub extern fn zh_curve_player_create(ctx: ?*Ctx, n_voices: u32, out: *?*CurvePlayer) c_int;" in zig
    assert "pub extern fn zh_curve_player_destroy(m: ?*CurvePlayer) c_int;" in zig
    assert "pub extern fn zh_curve_player_get_state(m: ?*CurvePlayer, host: ?[*]CurvePlayerState) c_int;" in zig
    assert "pub extern fn zh_curve_player_set_state(m: ?*CurvePlayer, host: ?[*]const CurvePlayerState) c_int;" in zig
    line = re.search(r"pub extern fn zh_curve_player_paint_spans\((.*?)\) c_int;", zig)
    assert line and "span_params: ?[*]const ScriptSpanParam" in line.group(1) and "params: ?*const CurvePlayerParams" in line.group(1)
    assert re.search(r"pub extern fn zh_curve_player_paint\(.*note_id_changed: Bool, params: \?\*const CurvePlayerParams, flags: u32\) c_int;", zig)
    assert "pub const CURVE_PLAYER_SPAN_FIELDS: u32 = 2;" in zig and "pub const CURVE_PLAYER_SPAN_EFFECT: u32 = 1;" in zig
    assert "pub const CurvePlayerParams = extern struct {" in zig and "pub const CurvePlayerState = extern struct {" in zig


def test_null_handles_are_refused():
    from zang_amd import abi
    lib = abi.load()
    e, h = abi.SfxEffect(), C.c_void_p()
    nodes = (abi.CurveNode * 9)()
    assert lib.zh_sfx_effect_curve_example(None, nodes) == abi.ZH_ERR_INVALID
    assert lib.zh_sfx_effect_curve_example(C.byref(e), None) == abi.ZH_ERR_INVALID
    assert lib.zh_curve_player_create(None, 4, C.byref(h)) == abi.ZH_ERR_INVALID and not h.value
    assert lib.zh_curve_player_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_curve_player_get_state(None, None) == abi.ZH_ERR_INVALID and lib.zh_curve_player_set_state(None, None) == abi.ZH_ERR_INVALID
    p = abi.CurvePlayerParams()
    assert lib.zh_curve_player_paint(None, 0, 0, None, None, abi.Bool(), C.byref(p), 0) == abi.ZH_ERR_INVALID
    assert lib.zh_curve_player_paint(None, 0, 0, None, None, abi.Bool(), None, 0) == abi.ZH_ERR_INVALID
    assert lib.zh_curve_player_paint_spans(None, 0, 0, None, None, C.byref(p), None, None, 0) == abi.ZH_ERR_INVALID


def test_example_effect_is_the_references_pair():
    """zh_sfx_effect_curve_example (no device): example_curve.zig:18-31 restated -- the modulator's three nodes, then the carrier's
    six, both smoothstep, no volume curve -- and what zang_amd.sfx holds"""
    from zang_amd import abi, sfx
    e = abi.SfxEffect()
    nodes = (abi.CurveNode * 9)()
    assert abi.load().zh_sfx_effect_curve_example(C.byref(e), nodes) == 0
    got = [(np.float32(nodes[i].t), np.float32(nodes[i].value)) for i in range(9)]
    assert got == [(np.float32(t), np.float32(v)) for t, v in sfx.CURVE_EXAMPLE_MODULATOR + sfx.CURVE_EXAMPLE_CARRIER]
    assert sfx.CURVE_EXAMPLE_CARRIER[-1] == (3.9, 20.0) and sfx.CURVE_EXAMPLE_MODULATOR[1] == (1.5, 55.0)
    base = C.addressof(nodes)
    assert (e.modulator.nodes, e.modulator.count, e.modulator.function) == (base, 3, sfx.smoothstep)
    assert (e.carrier.nodes, e.carrier.count, e.carrier.function) == (base + 24, 6, sfx.smoothstep)
    assert (e.volume.nodes, e.volume.count, e.volume.function) == (None, 0, sfx.smoothstep)
    m, c, v = sfx.curve_example_effect()
    assert m == (sfx.CURVE_EXAMPLE_MODULATOR, sfx.smoothstep) and c == (sfx.CURVE_EXAMPLE_CARRIER, sfx.smoothstep) and v == ([], sfx.smoothstep)


def test_the_kits_handle_is_defined_alike_in_both_translation_units():
    """curve_player.hip reads the kit through a second definition of laser.hip's struct zh_sfx_kit: the two texts are one"""
    body = lambda name: re.search(r"^struct zh_sfx_kit \{.*?^\};", open(os.path.join(CSRC, name)).read(), flags=re.S | re.M).group(0)
    assert body("curve_player.hip") == body("laser.hip")


def test_player_push_builds_the_note_records_without_a_device():
    """CurvePlayer.push: rel_freq, the effect index and an always-set note_on word per impulse, in push order"""
    from zang_amd import sfx

    class _Bank:
        def __init__(self):
            self.calls = []

        def push(self, *a):
            self.calls.append(a)
    p = object.__new__(sfx.CurvePlayer)
    p.bank = _Bank()
    p.push(2, 17, 5, 3, 1.1)
    p.push([0, 1], [0, 255], [6, 7], [0, 4], [0.9, 1.0])
    p.push([0, 1], [0, 255], [6, 7], 1, [0.5, 2.0])
    (a, b, c) = p.bank.calls
    assert a[:3] == (2, 17, 5) and a[3].dtype == sfx.CURVE_NOTE_PARAMS and len(a[3]) == 1
    assert a[3][0].tolist() == (np.float32(1.1), 3, 1)
    assert b[3]["effect"].tolist() == [0, 4] and b[3]["note_on"].tolist() == [1, 1] and b[3]["rel_freq"].tolist() == [np.float32(0.9), 1.0]
    assert c[3]["effect"].tolist() == [1, 1] and c[3]["rel_freq"].tolist() == [0.5, 2.0]


# ------------------------------------------------------------------ the yardstick's own check
def _example_kit():
    from zang_amd import sfx
    return cr.Kit([sfx.curve_example_effect()])


def test_reference_frequency_row_is_the_curve_times_rel_freq(oracle):
    """a voice started with note_id_changed over four buffers of 1,024 frames: its out1 row == the oracle Curve's own output
    (the carrier's nodes, smoothstep, into zeros) times rel_freq; out0 stays within the sum of one sine per paint; an effect index
    equal to the count touches nothing"""
    kit = _example_kit()
    voice = cr.Voice(oracle)
    L = oracle.lib()
    F, B, rel = 1024, 4, np.float32(1.5)
    out0, out1, want = (np.zeros(B * F, np.float32) for _ in range(3))
    temps = [np.zeros(B * F, np.float32) for _ in range(2)]
    alone = oracle.CurveModule()
    L.zo_curve_init(C.byref(alone))
    ptr, n, fn, _ = kit.curve(oracle, 0, 1)
    for b in range(B):
        cr.curve_player_paint(oracle, voice, kit, b * F, (b + 1) * F, out0, out1, temps, b == 0, cc.SR, rel, 0)
        L.zo_curve_paint(C.byref(alone), b * F, (b + 1) * F, oracle.fptr(want), int(b == 0), cc.SR, fn, ptr, n)
    L.zo_multiply_with_scalar(0, B * F, oracle.fptr(want), float(rel))
    assert cc.same_bits(out1, want) and out1[0] == np.float32(440.0) * rel and np.abs(out1).min() > 0
    assert 0.5 < np.abs(out0).max() <= 1.0
    before, words = (out0.copy(), out1.copy()), voice.words()
    cr.curve_player_paint(oracle, voice, kit, 0, F, out0, out1, temps, True, cc.SR, rel, 1)
    assert cc.same_bits(out0, before[0]) and cc.same_bits(out1, before[1]) and voice.words() == words


def test_reference_one_sub_span_equals_three(oracle):
    """the example's effect over [0, 256) in one sub-span == in the three sub-spans [0, 1), [1, 2), [2, 256) with note_id_changed
    clear after the first: both rows and the ten words, on bits.  The cuts are where the reference itself is exact: a Curve
    restarts its segment's accumulator at every paint from the quotient frames_in / segment_frames, and up to frame 2 the running
    sum of the step (s, s + s) IS that quotient; neither phase has reached 1 by then, so the wrap after a sub-span changes nothing.
    (At a later cut the quotient and the running sum part by an ulp -- the oracle, measured: cuts at 64 and 128 change one frame
    of the frequency row -- so no other three-way cut is held to bits here.)"""
    kit = _example_kit()
    rows = []
    for cuts in ([(0, 256)], [(0, 1), (1, 2), (2, 256)]):
        voice = cr.Voice(oracle)
        out0, out1 = np.zeros(256, np.float32), np.zeros(256, np.float32)
        temps = [np.zeros(256, np.float32) for _ in range(2)]
        for j, (s, e) in enumerate(cuts):
            cr.curve_player_paint(oracle, voice, kit, s, e, out0, out1, temps, j == 0, cc.SR, 1.0, 0)
        rows.append((out0, out1, voice.words()))
    (a0, a1, aw), (b0, b1, bw) = rows
    assert cc.same_bits(a0, b0) and cc.same_bits(a1, b1) and aw == bw
    assert np.abs(a0).max() > 0.5 and len(set(a1.tolist())) > 200


def test_the_test_tables_reach_every_case_the_issue_names():
    effects = cc.kit_effects()
    assert len(effects) == cc.N_EFFECTS == 5
    assert all(len(e[2][0]) == 0 for e in effects)                               # every volume curve is empty
    assert [fn for _, fn in effects[0][:2]] == [cc.SMOOTHSTEP, cc.SMOOTHSTEP]    # (a)
    assert any(e[1][1] == cc.LINEAR and len(e[1][0]) > 1 for e in effects)       # (b) a linear carrier
    assert any(len(e[0][0]) == 0 and len(e[1][0]) > 0 for e in effects)          # (c) an empty modulator curve
    assert any(len(e[0][0]) == 1 and len(e[1][0]) == 1 for e in effects)         # (d) single nodes
    dense = [e[1][0] for e in effects if len(e[1][0]) > 36]
    assert dense and all(len(c) == 40 and round(c[39][0] * cc.SR) == 78 for c in dense)   # (e) 40 nodes two frames apart
    V = 130
    tb = cc.tables(V, 1000 * V)
    walk = cc.walked(tb, V)
    assert {w[5] for w in walk} == set(range(6))
    assert any(w[5] == 5 and w[4] == 1 for w in walk)                            # the count as an index, note_id_changed set
    assert any(w[5] == 4 and w[3] - w[2] > 80 for w in walk)                     # the dense carrier in a sub-span longer than its nodes
    assert any(w[2] == w[3] for w in walk) and set(tb["count"].tolist()) == {0, 1, 2, 3, 4}
    assert tb["count"][4] == 0 and tb["start"][1, 1] < tb["end"][0, 1]           # no sub-span; the out-of-order one
    assert [w[1] for w in walk if w[0] == 1] == [0]                              # ... ends voice 1's list
    assert {(w[2], w[3]) for w in walk if w[0] == 0} == {(3, 51), (51, 51), (51, 195), (195, 250)}   # adjacent, empty, both edges
    assert tb["nic"][2, 0] == 0 and tb["effect"][2, 0] != tb["effect"][0, 0] and tb["end"][0, 0] - tb["start"][0, 0] == 48
    for seed in (1000 * V + 1,):
        second = cc.tables(V, seed, second=True)
        assert not second["nic"][0].any()
        for v in range(V):                                                       # another effect than the voice's last, note_id_changed clear
            if tb["count"][v]:
                assert second["effect"][0, v] != tb["effect"][tb["count"][v] - 1, v]
    for v in (1, 64, 65):                                                        # the smaller shapes keep the fixed patterns they can hold
        assert cc.tables(v, 1000 * v)["count"][0] == 4
    base = cc.base_image(8, 1)
    assert (base.view(np.uint32) == 0x80000000).sum() > 100 and (base[1::2, 200:].view(np.uint32) == 0x80000000).all()
