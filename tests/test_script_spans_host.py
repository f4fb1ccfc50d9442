"""CPU: the per-voice sub-span form of generated script modules (ZH_ZSCRIPT_FORM_SPANS, zh_script_module_paint_spans) --
the emitter adds zs_paint_spans_<name> for every module and leaves the lane kernels' text as it was, the new form compiles for
gfx950 (hiprtc needs no GPU), the two new structs have the C compiler's layout in the ctypes mirror, and ScriptSpanTable lays out
hand-made lists and zh_poly_voice schedules as the [span][voice] arrays the kernel reads."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import script_fuzz
from tests.hostprog import c_ints, c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = [os.path.join(ROOT, "tests", "golden", "script_modules.txt"), os.path.join(ROOT, "tests", "golden", "example_script.txt")]
SPANS_KERNEL = re.compile(r'\n\nextern "C" __global__ void __launch_bounds__\(64\) zs_paint_spans_(\w+)\(const ZsLaunch L, const ZsSpans S\) \{\n.*?\n\}\n', re.S)


def _generate(path, forms):
    from zang_amd import zscript_native as native
    nat = native.NativeScript(open(path).read(), os.path.basename(path))
    try:
        return nat.generate_hip(forms=forms)
    finally:
        nat.close()


@pytest.mark.parametrize("path", CORPUS, ids=["script_modules", "example_script"])
def test_spans_form_adds_a_kernel_per_module_and_leaves_the_lane_kernels_alone(path):
    from zang_amd import zscript_native as native
    plain, meta0 = _generate(path, 0)
    spans, meta = _generate(path, native.FORM_SPANS)
    assert meta == meta0
    refused = sorted(n for n, m in meta.items() if "error" in m)
    assert refused == [], refused                                   # nothing the lane form takes is refused by the spans form
    assert sorted(SPANS_KERNEL.findall(spans)) == sorted(meta)      # one per exported module
    assert SPANS_KERNEL.sub("\n", spans) == plain
    assert "zs_paint_spans_" not in plain


def test_spans_kernel_runs_the_prologue_per_sub_span():
    """params, NIC, the sub-span's start and length and every begin() are assigned in zs_begin; the state loads are not; frame
    positions are relative to the lane's sub-span"""
    from zang_amd import zscript_native as native
    text, _ = _generate(CORPUS[0], native.FORM_SPANS)
    k = SPANS_KERNEL.search(text[text.index("zs_paint_spans_Jingle") - 200:]).group(0)
    begin = k[k.index("auto zs_begin"):k.index("auto zs_end")]
    assert "m1.t = zs_ld_f(L.state" not in begin and "zs_ld_" not in begin
    assert "P0 = zs_span_f(L.p[0], S.p[0], zs_kv, v);" in begin and ".begin(" in begin and "SPAN_LEN = S.t.end[zs_kv] - zs_s0;" in begin
    assert "L.start" not in k and "(i - zs_s0)" in k
    assert "ZS_T" not in k                                          # exact only


def test_spans_form_compiles_for_gfx950():
    from zang_amd import script
    from zang_amd import zscript_native as native
    for path in CORPUS:
        src, _ = _generate(path, native.FORM_SPANS)
        assert script.compile_hip(src) > 10000


@pytest.mark.parametrize("seed", range(20))
def test_spans_form_of_random_scripts_compiles_for_gfx950(seed):
    from zang_amd import script
    from zang_amd import zscript_native as native
    text, name = script_fuzz.generate(seed)
    nat = native.NativeScript(text, "fuzz")
    src, meta = nat.generate_hip(only=[name], forms=native.FORM_SPANS)
    nat.close()
    assert "error" not in meta[name] and "zs_paint_spans_" + name in src
    assert script.compile_hip(src) > 1000


def test_struct_layouts_match_the_c_compiler():
    from zang_amd import abi
    T, P = abi.ScriptSpanTable, abi.ScriptSpanParam
    lay = c_layout({"zh_script_span_table": ["max_spans", "count", "start", "end", "note_id_changed"], "zh_script_span_param": ["f", "u"]})
    assert lay["zh_script_span_table"] == (C.sizeof(T), {"max_spans": T.max_spans.offset, "count": T.count.offset, "start": T.start.offset,
                                                         "end": T.end.offset, "note_id_changed": T.note_id_changed.offset})
    assert lay["zh_script_span_param"] == (C.sizeof(P), {"f": P.f.offset, "u": P.u.offset})
    assert c_ints(["ZH_ZSCRIPT_FORM_SPANS"]) == [abi.ZSCRIPT_FORM_SPANS]
    from zang_amd import zscript_native as native
    assert native.FORM_SPANS == abi.ZSCRIPT_FORM_SPANS


SPEC = [("sample_rate", "constant", None), ("freq", "constant_or_buffer", None), ("note_on", "boolean", None),
        ("ftype", "one_of", "FilterType"), ("k", "constant", None), ("x", "buffer", None)]


def test_span_table_from_hand_made_lists():
    from zang_amd import script
    lists = [
        [],                                                                          # count 0
        [(0, 100, True, {"freq": 440.0, "note_on": True, "k": 1.0}), (100, 100, False, {"freq": 440.0, "note_on": True, "k": 1.0}),
         (100, 1024, False, {"freq": 220.0, "note_on": False, "k": 1.0})],            # an empty interior sub-span
        [(5, 1024, True, {"freq": 330.0, "note_on": True, "k": 1.0}), (1024, 1024, True, {"freq": 331.0, "note_on": True, "k": 1.0})],   # empty at the end
        [(0, 300, False, {"freq": 440.0, "note_on": True, "k": 1.0, "ftype": ("notch", None)}),                                          # trigger_test.zig's
         (300, 1024, True, {"freq": 550.0, "note_on": True, "k": 1.0, "ftype": ".high_pass"})],                                          # carry-over pattern
    ]
    t = script.ScriptSpanTable.from_lists(SPEC, lists)
    assert t.max_spans == 3 and t.n_voices == 4
    assert t.count.tolist() == [0, 3, 2, 2]
    assert t.start.tolist() == [[0, 0, 5, 0], [0, 100, 1024, 300], [0, 100, 0, 0]]
    assert t.end.tolist() == [[0, 100, 1024, 300], [0, 100, 1024, 1024], [0, 1024, 0, 0]]
    assert t.note_id_changed.tolist() == [[0, 1, 1, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    assert sorted(t.arrays) == ["freq", "ftype", "note_on"]                         # k is the same everywhere: no array
    assert t.constants == {"k": 1.0}
    f, u = t.arrays["freq"]
    assert u is None and f.dtype == np.float32 and f.tolist() == [[0, 440, 330, 440], [0, 440, 331, 550], [0, 220, 0, 0]]
    f, u = t.arrays["note_on"]
    assert f is None and u.tolist() == [[0, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]]
    f, u = t.arrays["ftype"]
    assert u.tolist() == [[0, 0, 0, 4], [0, 0, 0, 3], [0, 0, 0, 0]] and f.tolist() == [[0] * 4] * 3
    with pytest.raises(ValueError):
        script.ScriptSpanTable.from_lists(SPEC, [[(0, 1, False, {"x": 1.0})]])     # a waveform does not vary per sub-span


def test_span_table_from_a_poly_voice_schedule():
    """zh_poly_voice_schedule's per-voice lists, computed here from its arrays, give the same table through both constructors"""
    from zang_amd import abi, script
    lib = abi.load()
    P, Fb, sr = 3, 1024, 44100.0
    dt = np.dtype({"names": ["freq", "note_on"], "formats": ["<f4", "u1"], "offsets": [0, 4], "itemsize": 8})
    ev = [(0.0, 1, 440.0, 1), (0.005, 2, 550.0, 1), (0.01, 1, 440.0, 0), (0.012, 3, 660.0, 1), (0.02, 4, 770.0, 1), (0.03, 2, 550.0, 0)]
    rec = np.zeros(len(ev), dt)
    for i, (_, _, f, on) in enumerate(ev):
        rec[i] = (f, on)
    t = np.array([e[0] for e in ev], np.float32); ids = np.array([e[1] for e in ev], np.uint64)
    h = C.c_void_p()
    abi.check(lib.zh_poly_voice_create(P, 8, 4, len(ev), rec.ctypes.data, t.ctypes.data, ids.ctypes.data, C.byref(h)), "zh_poly_voice_create")
    cap = 34
    count = np.zeros(P, np.uint32); start = np.zeros((cap, P), np.uint32); end = np.zeros((cap, P), np.uint32)
    params = np.zeros((cap, P), dt); nic = np.zeros((cap, P), np.uint8)
    fr = np.array([Fb], np.uint32)
    abi.check(lib.zh_poly_voice_schedule(h, sr, fr.ctypes.data, 1, cap, count.ctypes.data, start.ctypes.data, end.ctypes.data,
                                         params.ctypes.data, nic.ctypes.data), "zh_poly_voice_schedule")
    lib.zh_poly_voice_destroy(h)
    assert count.sum() >= 4
    lists = [[(int(start[k, v]), int(end[k, v]), bool(nic[k, v]), {"freq": float(params["freq"][k, v]), "note_on": bool(params["note_on"][k, v])})
              for k in range(int(count[v]))] for v in range(P)]
    spec = [("sample_rate", "constant", None), ("freq", "constant_or_buffer", None), ("note_on", "boolean", None)]
    a = script.ScriptSpanTable.from_lists(spec, lists)
    K = int(count.max())
    b = script.ScriptSpanTable(spec, count, start[:K], end[:K], nic[:K],
                               {"freq": (params["freq"][:K], None), "note_on": (None, params["note_on"][:K].astype(np.uint32))})
    assert a.max_spans == b.max_spans == K
    for name in ("count", "start", "end", "note_id_changed"):
        x, y = getattr(a, name), getattr(b, name)
        mask = np.arange(K)[:, None] < count[None, :] if x.ndim == 2 else np.ones_like(x, bool)
        assert np.array_equal(np.where(mask, x, 0), np.where(mask, y, 0)), name
    for name in ("freq", "note_on"):
        i = 0 if name == "freq" else 1
        mask = np.arange(K)[:, None] < count[None, :]
        assert np.array_equal(np.where(mask, a.arrays[name][i], 0), np.where(mask, b.arrays[name][i], 0)), name
    # Trigger's sub-spans of a voice: ascending, inside the buffer, note_id_changed where a new note starts
    for v in range(P):
        spans = lists[v]
        assert all(0 <= s <= e <= Fb for s, e, _, _ in spans)
        assert all(spans[j][1] <= spans[j + 1][0] for j in range(len(spans) - 1))
