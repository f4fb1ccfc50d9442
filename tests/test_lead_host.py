"""CPU: the two lead voices without a device.  The surface -- the header, the ctypes mirror and the Zig binding declare the
fourteen entry points and both field enums, struct sizes and offsets agree with gcc, NULL handles are refused, the state layouts
pack and unpack under AddressSanitizer + UBSan (a stand-alone program with its own main: nothing loaded into python runs under a
sanitizer) -- the portamento example's key rule alone, and the yardstick's own checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import lead_cases as lc
from tests import lead_reference as lr
from tests.hostprog import flat_header, mirror_layout, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_SRC = os.path.join(ROOT, "tests", "cpp", "lead_state_host.cpp")
NAMES = ("porta", "vibrato")


def _decls(x):
    return [
        f"ZH_API int zh_{x}_patch_default(zh_{x}_patch *patch);",
        f"ZH_API int zh_{x}_create(zh_ctx *ctx, uint32_t n_voices, zh_{x} **out);",
        f"ZH_API int zh_{x}_destroy(zh_{x} *m);",
        f"ZH_API int zh_{x}_get_state(zh_{x} *m, zh_{x}_state *host);",
        f"ZH_API int zh_{x}_set_state(zh_{x} *m, const zh_{x}_state *host);",
        f"ZH_API int zh_{x}_paint(zh_{x} *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
        f"zh_bool note_id_changed, const zh_{x}_params *params, uint32_t flags);",
        f"ZH_API int zh_{x}_paint_spans(zh_{x} *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, "
        f"const zh_{x}_params *params, const zh_script_span_param *span_params, const zh_script_span_table *table, uint32_t flags);",
    ]


FIELDS = ["FREQ", "NOTE_ON"]
PATCH_FIELDS = {"porta": ["glide_curve", "glide", "attack", "decay", "release", "sustain_volume"], "vibrato": ["vib_hz", "depth", "color"]}
STATE_FIELDS = {"porta": ["porta", "env", "osc", "prev_note_on"], "vibrato": ["vib", "osc"]}


@pytest.mark.parametrize("x", NAMES)
def test_header_declares_the_entry_points_and_the_field_enum(x):
    text = flat_header()
    for decl in _decls(x):
        assert " ".join(decl.split()) in text, decl
    X = x.upper()
    m = re.search(r"enum \{ (ZH_%s_SPAN_FREQ = 0.*?) \};" % X, text)
    assert m, f"no ZH_{X}_SPAN_* enum"
    names = [n.strip().split(" ")[0] for n in m.group(1).split(",")]
    assert names == [f"ZH_{X}_SPAN_" + f for f in FIELDS] + [f"ZH_{X}_SPAN_FIELDS"]
    state = re.search(r"typedef struct zh_%s_state \{(.*?)\} zh_%s_state;" % (x, x), text).group(1)
    assert [s.split()[-1] for s in state.split(";") if s.strip()] == STATE_FIELDS[x]


@pytest.mark.parametrize("x", NAMES)
def test_ctypes_mirror_and_python_fields_follow_the_header(x):
    from zang_amd import abi, lead, modules as mod
    P, vp, u32 = C.POINTER, C.c_void_p, C.c_uint32
    N = x.capitalize()
    patch_t, params_t, state_t = (getattr(abi, N + s) for s in ("Patch", "Params", "State"))
    cls = getattr(mod, N)
    assert abi.SIGNATURES[f"zh_{x}_patch_default"] == (C.c_int, [P(patch_t)])
    assert abi.SIGNATURES[f"zh_{x}_create"] == (C.c_int, [vp, u32, P(vp)])
    assert abi.SIGNATURES[f"zh_{x}_destroy"] == (C.c_int, [vp])
    for name in (f"zh_{x}_get_state", f"zh_{x}_set_state"):
        assert abi.SIGNATURES[name] == (C.c_int, [vp, vp])
    assert abi.SIGNATURES[f"zh_{x}_paint"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), abi.Bool, P(params_t), u32])
    assert abi.SIGNATURES[f"zh_{x}_paint_spans"] == (C.c_int, [vp, u32, u32, P(abi.Buf), P(abi.Buf), P(params_t),
                                                               P(abi.ScriptSpanParam), P(abi.ScriptSpanTable), u32])
    for i, f in enumerate(FIELDS):
        assert getattr(abi, f"{x.upper()}_SPAN_" + f) == i
    assert getattr(abi, f"{x.upper()}_SPAN_FIELDS") == 2
    assert [n.upper() for n, _ in cls._span_fields] == FIELDS == [n.upper() for n in lr.FIELDS]
    assert [n for n, _ in state_t._fields_] == STATE_FIELDS[x]
    ref_patch = lr.PortaPatch if x == "porta" else lr.VibratoPatch
    assert [n for n, _ in patch_t._fields_] == PATCH_FIELDS[x] == list(ref_patch.__dataclass_fields__) == list(cls.Patch.__dataclass_fields__)
    assert [n for n, _ in params_t._fields_] == ["sample_rate", "reserved", "freq", "note_on", "patch"]
    assert [n for n in lead.NOTE_PARAMS.names] == [n for n, _ in lr.Note._fields_] and lead.NOTE_PARAMS.itemsize == C.sizeof(lr.Note)
    assert getattr(abi.load(), f"zh_{x}_paint_spans").argtypes is not None


def test_struct_sizes_and_offsets_match_gcc():
    from zang_amd import abi
    names = {f"zh_{x}_{s}": getattr(abi, x.capitalize() + s.capitalize()) for x in NAMES for s in ("patch", "params", "state")}
    _, seen = mirror_layout(names)
    assert seen == 6 + (6 + 5 + 4) + (3 + 5 + 2)
    assert C.sizeof(abi.PortaState) == 36 and C.sizeof(abi.VibratoState) == 8 and C.sizeof(abi.PortaPatch) == 24 and C.sizeof(abi.VibratoPatch) == 12


def test_zig_binding_declares_them():
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    for x in NAMES:
        N = x.capitalize()
        assert f"pub extern fn zh_{x}_create(ctx: ?*Ctx, n_voices: u32, out: *?*{N}) c_int;" in zig
        assert f"pub extern fn zh_{x}_patch_default(patch: ?*{N}Patch) c_int;" in zig
        line = re.search(r"pub extern fn zh_%s_paint_spans\((.*?)\) c_int;" % x, zig)
        assert line and "span_params: ?[*]const ScriptSpanParam" in line.group(1) and f"params: ?*const {N}Params" in line.group(1)
        assert re.search(r"pub extern fn zh_%s_paint\(.*note_id_changed: Bool, params: \?\*const %sParams, flags: u32\) c_int;" % (x, N), zig)
        assert f"pub const {x.upper()}_SPAN_FIELDS: u32 = 2;" in zig and f"pub const {x.upper()}_SPAN_NOTE_ON: u32 = 1;" in zig
        assert f"pub const {N}Params = extern struct {{" in zig and f"pub const {N}State = extern struct {{" in zig
        for name in ("destroy", "get_state", "set_state"):
            assert f"pub extern fn zh_{x}_{name}(" in zig


@pytest.mark.parametrize("x", NAMES)
def test_null_handles_are_refused_and_the_default_patch_is_the_references(x):
    from zang_amd import abi
    lib = abi.load()
    fn = lambda name: getattr(lib, f"zh_{x}_{name}")
    N = x.capitalize()
    h = C.c_void_p()
    assert fn("create")(None, 4, C.byref(h)) == abi.ZH_ERR_INVALID
    assert fn("destroy")(None) == abi.ZH_ERR_INVALID
    assert fn("get_state")(None, None) == abi.ZH_ERR_INVALID and fn("set_state")(None, None) == abi.ZH_ERR_INVALID
    p = getattr(abi, N + "Params")()
    assert fn("paint")(None, 0, 0, None, None, abi.Bool(), C.byref(p), 0) == abi.ZH_ERR_INVALID
    assert fn("paint_spans")(None, 0, 0, None, None, C.byref(p), None, None, 0) == abi.ZH_ERR_INVALID
    assert fn("patch_default")(None) == abi.ZH_ERR_INVALID
    patch = getattr(abi, N + "Patch")()
    assert fn("patch_default")(C.byref(patch)) == 0
    ref = lr.PortaPatch() if x == "porta" else lr.VibratoPatch()
    for f in PATCH_FIELDS[x]:                                        # example_portamento.zig:57, :68-71; example_vibrato.zig:49, :54, :61
        assert np.float32(getattr(patch, f)) == np.float32(getattr(ref, f)), f


def test_state_layouts_under_the_sanitizers(tmp_path):
    """0, 1, 65 and 130 voices of both leads -- and of the four other voices on the same host side: HardSquare, SawEnv, detuned,
    laser -- packed into heap blocks of exactly the library's size and read back: every word written once, at [word][voice]; every
    field of the six state structs back on bits"""
    run_sanitized(STATE_SRC, tmp_path)


# ------------------------------------------------------------------ the key rule alone
KEY_FREQS = (55.0 * 2.0 ** (np.arange(64) / 12.0)).astype(np.float32)
# (key_index, down) -> what the reference's keyEvent pushes (freq key, note_on), or None
SCRIPT = [((10, True), (10, True)),              # the first key
          ((20, True), (20, True)),              # a higher one: pushed
          ((5, True), None),                     # a lower key under a higher one: no push
          ((20, True), None),                    # a repeated key down
          ((20, False), (10, True)),             # the highest released with others held: note-on at the next highest
          ((63, True), (63, True)),              # key index 63
          ((10, False), (63, True)),             # a lower key released: the highest held sounds again
          ((63, False), (5, True)),
          ((5, False), (5, False)),              # the last key released: note-off
          ((0, True), (0, True)),                # key index 0 after silence
          ((0, False), (0, False))]


def test_the_key_rule_alone():
    from zang_amd import lead
    ours, theirs = lead.PortaKeys(KEY_FREQS), lr.PortaKeys(KEY_FREQS)
    ids, on_id = [], None
    for (key, down), want in SCRIPT:
        got, ref = ours.key(key, down), theirs.key_event(key, down)
        if want is None:
            assert got is None and ref is None, (key, down, got, ref)
            continue
        assert ref[1:] == (KEY_FREQS[want[0]], want[1]), (key, down, ref)
        assert got[1:] == (float(KEY_FREQS[want[0]]), want[1]), (key, down, got)
        if want[1]:
            assert got[0] == ref[0]                                  # a fresh id per push, in step with the reference's IdGenerator
            on_id = got[0]
        else:
            assert got[0] == on_id                                   # a note-off goes out under the id of the note that is on
        ids.append(ref[0])
        assert ours.keys_held == theirs.keys_held
    assert ids == list(range(1, 10)) and ours.keys_held == 0
    with pytest.raises(ValueError):
        ours.key(64, True)
    with pytest.raises(ValueError):
        lead.PortaKeys(np.zeros(65, np.float32))


def test_player_push_builds_the_note_record():
    from zang_amd import lead

    class _Bank:
        def __init__(self):
            self.calls = []

        def push(self, *a):
            self.calls.append(a)
    p = object.__new__(lead.PortaPlayer)
    p.bank, p.keys = _Bank(), [lead.PortaKeys(KEY_FREQS) for _ in range(2)]
    assert p.key(1, 12, True, 17) == (1, float(KEY_FREQS[12]), True) and p.key(1, 3, True, 18) is None
    p.push([0, 1], [0, 255], [6, 7], [330.0, 110.0], [False, True])
    (a, b) = p.bank.calls
    assert a[:3] == (1, 17, 1) and a[3].dtype == lead.NOTE_PARAMS and a[3][0].tolist() == (float(KEY_FREQS[12]), 1)
    assert b[3]["freq"].tolist() == [330.0, 110.0] and b[3]["note_on"].tolist() == [0, 1]


# ------------------------------------------------------------------ the yardstick's own checks
@pytest.mark.parametrize("kind", lc.KINDS, ids=lc.KIND_IDS)
def test_reference_span_form_over_one_full_sub_span_is_its_plain_paint(oracle, kind):
    V = 6
    S, E = lc.SPAN
    tb = lc.one_span_tables(V, 9)
    a, b = kind.voices(oracle, V), kind.voices(oracle, V)
    base, sync0 = lc.base_image(V, 1), lc.base_image(V, 2)
    img, sync = base.copy(), sync0.copy()
    lr.paint_spans(oracle, kind.paint, a, tb, img, sync, lc.SPAN, lc.SR, False, kind.test_patch)
    plain, psync = base.copy(), sync0.copy()
    temps = [np.zeros(lc.ROWS, np.float32) for _ in range(3)]
    for v in range(V):
        kind.paint(oracle, b[v], S, E, (plain[v], psync[v]), temps, tb["nic"][0, v], lc.SR, tb["freq"][0, v], tb["note_on"][0, v], kind.test_patch)
    assert lc.same_bits(img, plain) and lc.same_bits(sync, psync)
    assert np.array_equal(lr.state_words(a), lr.state_words(b))
    assert lc.same_bits(plain[:, :S], base[:, :S]) and lc.same_bits(plain[:, E:], base[:, E:]) and not lc.same_bits(plain, base)
    assert np.abs(plain - base).max() > 0.05 and (psync - sync0)[:, S:E].min() > 50.0        # a voice, and its frequency beside it


def test_the_test_tables_reach_every_case_the_issue_names():
    for V in (1, 64, 65, 130):
        tbs = [lc.tables(V, 1000 * V + b, note_on_first=b == 0) for b in range(2)]
        assert lc.covers_every_pair(tbs), (V, lc.pairs(tbs))
    tb = lc.tables(130, 130000)
    live = np.arange(lc.MAX_SPANS)[:, None] < tb["count"][None, :]
    assert (live & (tb["start"] == tb["end"])).any() and set(tb["count"].tolist()) == {0, 1, 2, 3, 4}
    assert tb["count"][4] == 0 and tb["start"][1, 1] < tb["end"][0, 1]           # no sub-span; the out-of-order one
    p = lc.PORTA.test_patch
    assert p.attack * lc.SR + p.decay * lc.SR < 51 - 3 and p.release * lc.SR < 100 and 15 <= p.glide * lc.SR <= 40
    base = lc.base_image(8, 1)
    assert (base.view(np.uint32) == 0x80000000).sum() > 100
    V, tb = lc.hostile_freq_tables()
    for i, x in enumerate(lc.HOSTILE_FREQ):
        for v in (64 * i, 64 * len(lc.HOSTILE_FREQ) + i):
            k = int(tb["count"][v]) - 1
            assert tb["start"][k, v] >= lc.HOSTILE_FROM and np.array_equal(tb["freq"][k, v], np.float32(x), equal_nan=True)
            assert np.isfinite(tb["freq"][:k, v]).all()
    assert (lc.SPAN[1] - lc.HOSTILE_FROM) / (lc.SPAN[1] - lc.SPAN[0]) < lc.NAN_CAP


@pytest.mark.parametrize("kind", lc.KINDS, ids=lc.KIND_IDS)
def test_reference_nan_share_of_hostile_freq_stays_under_the_cap(oracle, kind):
    V, tb = lc.hostile_freq_tables()
    voices = kind.voices(oracle, V)
    ref, rsync = lc.base_image(V, 90), lc.base_image(V, 91)
    lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, False, kind.test_patch)
    assert 0.0 < lc.worst_row_nan_share(ref, rsync) <= lc.NAN_CAP
