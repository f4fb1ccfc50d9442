"""CPU: the detuned voice without a device.  The surface -- the header, the ctypes mirror and the Zig binding declare the entry
points and the three-field enum, struct sizes and offsets agree with gcc, NULL handles are refused, Detuned._paint_spans and
DetunedPlayer.push build the right ctypes arguments -- and the yardstick's own checks: tests/detuned_reference.py's span form
over one full sub-span is its plain paint, the planted warble reaches pow's arms, the NaN shares the GPU tests cap."""
import ctypes as C
import os
import re

import numpy as np

from tests import detuned_cases as dc
from tests import detuned_reference as dr
from tests.hostprog import flat_header, mirror_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = [
    "ZH_API int zh_detuned_patch_default(zh_detuned_patch *patch);",
    "ZH_API int zh_detuned_create(zh_ctx *ctx, uint32_t n_voices, uint64_t first_seed, zh_detuned **out);",
    "ZH_API int zh_detuned_destroy(zh_detuned *m);",
    "ZH_API int zh_detuned_get_state(zh_detuned *m, zh_detuned_state *host);",
    "ZH_API int zh_detuned_set_state(zh_detuned *m, const zh_detuned_state *host);",
    "ZH_API int zh_detuned_paint(zh_detuned *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "zh_bool note_id_changed, const zh_detuned_params *params, uint32_t flags);",
    "ZH_API int zh_detuned_paint_spans(zh_detuned *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
    "const zh_detuned_params *params, const zh_script_span_param *span_params, const zh_script_span_table *table, uint32_t flags);",
]
FIELDS = ["FREQ", "NOTE_ON", "MODE"]
PATCH_FIELDS = ["warble_hz", "warble_wide", "color", "volume", "attack", "decay", "release", "sustain_volume", "cutoff_hz", "res"]


def test_header_declares_the_entry_points_and_the_field_enum():
    text = flat_header()
    for decl in DECLS:
        assert " ".join(decl.split()) in text, decl
    m = re.search(r"enum \{ (ZH_DETUNED_SPAN_FREQ = 0.*?) \};", text)
    assert m, "no ZH_DETUNED_SPAN_* enum"
    names = [x.strip().split(" ")[0] for x in m.group(1).split(",")]
    assert names == ["ZH_DETUNED_SPAN_" + f for f in FIELDS] + ["ZH_DETUNED_SPAN_FIELDS"]
    state = re.search(r"typedef struct zh_detuned_state \{(.*?)\} zh_detuned_state;", text).group(1)
    assert [x.split()[-1] for x in state.split(";") if x.strip()] == ["noise", "noise_filter", "osc", "env", "main_filter"]


def test_ctypes_mirror_and_python_fields_follow_the_header():
    from zang_amd import abi, detuned, modules as mod
    P, vp, u32, u64 = C.POINTER, C.c_void_p, C.c_uint32, C.c_uint64
    assert abi.SIGNATURES["zh_detuned_patch_default"] == (C.c_int, [P(abi.DetunedPatch)])
    assert abi.SIGNATURES["zh_detuned_create"] == (C.c_int, [vp, u32, u64, P(vp)])
    assert abi.SIGNATURES["zh_detuned_destroy"] == (C.c_int, [vp])
    for name in ("zh_detuned_get_state", "zh_detuned_set_state"):
        assert abi.SIGNATURES[name] == (C.c_int, [vp, vp])
    assert abi.SIGNATURES["zh_detuned_paint"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), abi.Bool, P(abi.DetunedParams), u32])
    assert abi.SIGNATURES["zh_detuned_paint_spans"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), P(abi.DetunedParams),
                                                                  P(abi.ScriptSpanParam), P(abi.ScriptSpanTable), u32])
    for i, f in enumerate(FIELDS):
        assert getattr(abi, "DETUNED_SPAN_" + f) == i
    assert abi.DETUNED_SPAN_FIELDS == 3
    assert [n.upper() for n, _ in mod.Detuned._span_fields] == FIELDS == [n.upper() for n in dr.FIELDS]
    assert [n for n, _ in abi.DetunedState._fields_] == ["noise", "noise_filter", "osc", "env", "main_filter"]
    assert [n for n, _ in abi.DetunedPatch._fields_] == PATCH_FIELDS == list(dr.Patch.__dataclass_fields__) == list(mod.Detuned.Patch.__dataclass_fields__)
    assert [n for n in detuned.NOTE_PARAMS.names] == [n for n, _ in dr.Note._fields_] and detuned.NOTE_PARAMS.itemsize == C.sizeof(dr.Note)
    assert abi.load().zh_detuned_paint_spans.argtypes is not None


def test_struct_sizes_and_offsets_match_gcc():
    from zang_amd import abi
    names = {"zh_detuned_patch": abi.DetunedPatch, "zh_detuned_params": abi.DetunedParams, "zh_detuned_state": abi.DetunedState}
    _, seen = mirror_layout(names)
    assert seen == 3 + 10 + 6 + 5 and C.sizeof(abi.DetunedState) == 104 and C.sizeof(abi.DetunedPatch) == 40


def test_zig_binding_declares_them():
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    assert "pub extern fn zh_detuned_create(ctx: ?*Ctx, n_voices: u32, first_seed: u64, out: *?*Detuned) c_int;" in zig
    assert "pub extern fn zh_detuned_patch_default(patch: ?*DetunedPatch) c_int;" in zig
    line = re.search(r"pub extern fn zh_detuned_paint_spans\((.*?)\) c_int;", zig)
    assert line and "span_params: ?[*]const ScriptSpanParam" in line.group(1) and "params: ?*const DetunedParams" in line.group(1)
    assert re.search(r"pub extern fn zh_detuned_paint\(.*note_id_changed: Bool, params: \?\*const DetunedParams, flags: u32\) c_int;", zig)
    assert "pub const DETUNED_SPAN_FIELDS: u32 = 3;" in zig and "pub const DETUNED_SPAN_MODE: u32 = 2;" in zig
    assert "pub const DetunedParams = extern struct {" in zig and "pub const DetunedState = extern struct {" in zig


def test_null_handles_are_refused_and_the_default_patch_is_the_references():
    from zang_amd import abi
    lib = abi.load()
    h = C.c_void_p()
    assert lib.zh_detuned_create(None, 4, 0, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_detuned_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_detuned_get_state(None, None) == abi.ZH_ERR_INVALID and lib.zh_detuned_set_state(None, None) == abi.ZH_ERR_INVALID
    p = abi.DetunedParams()
    assert lib.zh_detuned_paint(None, 0, 0, None, None, abi.Bool(), C.byref(p), 0) == abi.ZH_ERR_INVALID
    assert lib.zh_detuned_paint_spans(None, 0, 0, None, None, C.byref(p), None, None, 0) == abi.ZH_ERR_INVALID
    assert lib.zh_detuned_patch_default(None) == abi.ZH_ERR_INVALID
    patch = abi.DetunedPatch()
    assert lib.zh_detuned_patch_default(C.byref(patch)) == 0
    for f in PATCH_FIELDS:                                           # example_detuned.zig:146, :153, :71, :76, :81-84, :95, :98
        assert np.float32(getattr(patch, f)) == np.float32(getattr(dr.Patch(), f)), f


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


def test_span_table_lays_out_what_the_entry_point_takes():
    """`freq` and `mode` vary per sub-span, note_on comes from the params: one zh_detuned_paint_spans call with the span and
    flags, TWO output bufs (the second NULL when no frequency image is given), the table's arrays, span_params in the C order."""
    from zang_amd import abi, modules as mod, zang
    m = object.__new__(mod.Detuned)
    m.lib, m.handle, m.ctx, m.n_voices = _FakeLib(), C.c_void_p(1234), _FakeCtx(), 4
    V = 4
    mode = np.array([[1, 2, 3, 0], [0, 1, 1, 1]], np.uint32)
    fr = np.full((2, V), 220.5, np.float32)
    table = m.span_table(np.array([1, 2, 0, 1]), np.array([[0, 0, 0, 10], [0, 512, 0, 0]]), np.array([[1024, 512, 0, 20], [0, 1024, 0, 0]]),
                         np.array([[1, 0, 0, 1], [0, 1, 0, 0]]), {"mode": (None, mode), "freq": (fr, None)})
    out = abi.Buf(0x2000, V, 1024, V, 0)
    patch = mod.Detuned.Patch(res=0.3)
    rc = m._paint_spans(zang.Span(16, 1000), [out], None, m.Params(48000.0, 330.0, True, 1, patch), table, abi.PAINT_ZERO_FIRST)
    assert rc == 0
    (args,) = m.lib.fns["zh_detuned_paint_spans"].calls
    handle, s, e, outs, temps, cp, sp, tb, flags = args
    assert (s, e, flags) == (16, 1000, abi.PAINT_ZERO_FIRST) and temps is None and handle.value == 1234
    assert len(outs) == 2 and outs[0].ptr == 0x2000 and outs[0].voices == V and not outs[1].ptr
    cp = cp._obj
    assert cp.sample_rate == 48000.0 and cp.freq.value == 330.0 and cp.note_on.value == 1 and cp.mode.value == 1
    assert cp.freq.per_voice is None and cp.mode.per_voice is None
    assert np.float32(cp.patch.res) == np.float32(0.3) and cp.patch.cutoff_hz == 880.0 and cp.patch.volume == 0.75
    tb = tb._obj
    assert tb.max_spans == 2
    assert np.ctypeslib.as_array(C.cast(tb.count, C.POINTER(C.c_uint32)), (V,)).tolist() == [1, 2, 0, 1]
    assert np.ctypeslib.as_array(C.cast(tb.note_id_changed, C.POINTER(C.c_uint8)), (2, V)).tolist() == [[1, 0, 0, 1], [0, 1, 0, 0]]
    assert sp[abi.DETUNED_SPAN_MODE].f is None
    assert np.ctypeslib.as_array(C.cast(sp[abi.DETUNED_SPAN_MODE].u, C.POINTER(C.c_uint32)), (2, V)).tolist() == mode.tolist()
    assert sp[abi.DETUNED_SPAN_FREQ].u is None
    assert np.ctypeslib.as_array(C.cast(sp[abi.DETUNED_SPAN_FREQ].f, C.POINTER(C.c_float)), (2, V)).tolist() == fr.tolist()
    assert sp[abi.DETUNED_SPAN_NOTE_ON].f is None and sp[abi.DETUNED_SPAN_NOTE_ON].u is None
    sync = abi.Buf(0x3000, V, 1024, V, 0)
    m._paint_spans(zang.Span(16, 1000), [out, sync], None, m.Params(48000.0), table, abi.PAINT_ADD)
    assert m.lib.fns["zh_detuned_paint_spans"].calls[1][3][1].ptr == 0x3000


def test_player_push_stores_the_mode_of_the_moment():
    """DetunedPlayer.push: freq, note_on and the player's CURRENT mode per impulse (example_detuned.zig:253-260)"""
    from zang_amd import detuned

    class _Bank:
        def __init__(self):
            self.calls = []

        def push(self, *a):
            self.calls.append(a)
    p = object.__new__(detuned.DetunedPlayer)
    p.bank, p.mode = _Bank(), 1
    p.push(2, 17, 5, 220.0, True)
    p.mode = 2
    p.push([0, 1], [0, 255], [6, 7], [330.0, 110.0], [False, True])
    (a, b) = p.bank.calls
    assert a[:3] == (2, 17, 5) and a[3].dtype == detuned.NOTE_PARAMS and a[3][0].tolist() == (220.0, 1, 1)
    assert b[3]["freq"].tolist() == [330.0, 110.0] and b[3]["note_on"].tolist() == [0, 1] and b[3]["mode"].tolist() == [2, 2]


# ------------------------------------------------------------------ the yardstick's own checks
def test_reference_span_form_over_one_full_sub_span_is_its_plain_paint(oracle):
    V = 6
    S, E = dc.SPAN
    tb = dc.one_span_tables(V, 9)
    a = [dr.Voice(oracle, dc.FIRST_SEED + v) for v in range(V)]
    b = [dr.Voice(oracle, dc.FIRST_SEED + v) for v in range(V)]
    base, sync0 = dc.base_image(V, 1), dc.base_image(V, 2)
    img, sync = base.copy(), sync0.copy()
    dr.paint_spans(oracle, a, tb, img, sync, dc.SPAN, dc.SR, False, dc.TEST_PATCH)
    plain, psync = base.copy(), sync0.copy()
    temps = [np.zeros(dc.ROWS, np.float32) for _ in range(4)]
    for v in range(V):
        dr.outer_paint(oracle, b[v], S, E, (plain[v], psync[v]), temps, tb["nic"][0, v], dc.SR, tb["freq"][0, v], tb["note_on"][0, v],
                       tb["mode"][0, v], dc.TEST_PATCH)
    assert dc.same_bits(img, plain) and dc.same_bits(sync, psync)
    assert np.array_equal(dr.state_words(a), dr.state_words(b))
    assert dc.same_bits(plain[:, :S], base[:, :S]) and dc.same_bits(plain[:, E:], base[:, E:]) and not dc.same_bits(plain, base)
    assert np.abs(plain - base).max() > 0.05 and (psync - sync0)[:, S:E].min() > 50.0        # a voice, and its frequency beside it


def test_reference_default_patch_sounds_and_releases(oracle):
    """the reference's constants over ten buffers of 256 frames: the attack's 1,200 frames end in the fifth, the decay (4,800) is
    cut short by a note-off in the seventh, the release (48,000) still runs in the tenth; the warble stays inside pow's
    fractional arm"""
    voice = dr.Voice(oracle, 7)
    F = 256
    temps = [np.zeros(F, np.float32) for _ in range(4)]
    states, peak = [], []
    for b in range(10):
        out, sync = np.zeros(F, np.float32), np.zeros(F, np.float32)
        dr.outer_paint(oracle, voice, 0, F, (out, sync), temps, b == 0, dc.SR, 220.0, b < 6, 0, dc.DEFAULT_PATCH)
        states.append(int(voice.env.state)); peak.append(float(np.abs(out).max()))
        assert np.abs(np.log2(sync / 220.0)).max() < 0.125
    assert states[0] == oracle.ENV_ATTACK and states[4] == states[5] == oracle.ENV_DECAY and states[6] == states[9] == oracle.ENV_RELEASE
    assert max(peak) > 0.1 and peak[9] > 0.0


def _planted_run(oracle, V):
    """V voices, the 22 planted ones first (each PLANTED value in mode 0, then in mode 1), one full sub-span"""
    voices = [dr.Voice(oracle, dc.FIRST_SEED + v) for v in range(V)]
    mode = np.zeros(V, np.uint32)
    for i, w in enumerate(dc.PLANTED + dc.PLANTED):
        voices[i].noise_filter.l = float(np.float32(w))
        mode[i] = i // len(dc.PLANTED)
    tb = dc.one_span_tables(V, 22)
    tb["mode"][0, :len(mode)] = mode
    img, sync = np.zeros((V, dc.ROWS), np.float32), np.zeros((V, dc.ROWS), np.float32)
    dr.paint_spans(oracle, voices, tb, img, sync, dc.SPAN, dc.SR, False, dc.TEST_PATCH)
    return img, sync


def test_planted_warble_reaches_every_arm_of_pow(oracle):
    S, E = dc.SPAN
    img, sync = _planted_run(oracle, 22)
    f = sync[:, S]                                                   # the first frame's frequency: freq * 2^w
    n = len(dc.PLANTED)
    with np.errstate(all="ignore"):
        assert np.isinf(f[dc.PLANTED.index(40.0)]) and np.isnan(img[dc.PLANTED.index(40.0), S + 1:E]).all()     # overflow, NaN from the second frame on
        assert f[dc.PLANTED.index(-160.0)] == 0.0                                                                 # underflow (mode 0: w = -640)
        assert 0.0 < f[dc.PLANTED.index(-37.4)] < 1.2e-38                                                         # denormal: 2^-149.6 x freq
        assert f[n + dc.PLANTED.index(7.6)] > 100.0 * 100.0 and f[n + dc.PLANTED.index(-7.6)] < 10.0              # the integer loop, the reciprocal arm
    assert np.isfinite(img[n + dc.PLANTED.index(31.9)]).all()
    assert 0.0 < dc.nan_share(img[:, S:E], sync[:, S:E]) < 0.25


def test_the_test_tables_reach_every_case_the_issue_names():
    tb = dc.tables(130, 130000)
    live = np.arange(dc.MAX_SPANS)[:, None] < tb["count"][None, :]
    assert set(tb["mode"][live].tolist()) == {0, 1, 2, 3} and set(tb["note_on"][live].tolist()) == {0, 1}
    assert (live & (tb["start"] == tb["end"])).any() and set(tb["count"].tolist()) == {0, 1, 2, 3, 4}
    assert tb["count"][4] == 0 and tb["start"][1, 1] < tb["end"][0, 1]           # no sub-span; the out-of-order one
    # the short patch: attack 15 + decay 25 frames end inside voice 0's first sub-span of 48, its release of 40 inside a later one
    assert dc.TEST_PATCH.attack * dc.SR + dc.TEST_PATCH.decay * dc.SR < 51 - 3 and dc.TEST_PATCH.release * dc.SR < 100
    base = dc.base_image(8, 1)
    assert (base.view(np.uint32) == 0x80000000).sum() > 100
