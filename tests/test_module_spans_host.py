"""CPU: the builtin modules' span paints (zh_<module>_paint_spans) at the ABI level -- the header declares them and their field
enums, the Zig binding and the ctypes mirror follow, and ModuleClass.paint_spans builds the right call without a device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zang_hip.h")
MODULES = ["sineosc", "pulseosc", "trisawosc", "noise", "envelope", "gate", "filter", "sampler", "decimator", "distortion"]
FIELDS = {   # the issue's table, in the C order
    "sineosc": ["FREQ", "PHASE"], "pulseosc": ["FREQ", "COLOR"], "trisawosc": ["FREQ", "COLOR"], "noise": ["COLOR"],
    "envelope": ["ATTACK", "DECAY", "RELEASE", "SUSTAIN_VOLUME", "NOTE_ON"], "gate": ["NOTE_ON"], "filter": ["TYPE", "CUTOFF", "RES"],
    "sampler": ["SAMPLE_RATE", "LOOP"], "decimator": ["FAKE_SAMPLE_RATE"], "distortion": ["TYPE", "INGAIN", "OUTGAIN", "OFFSET"],
}


def _enum_values(text, prefix):
    """{name: value} of the enum constants ZH_<prefix>_* (implicit values counted)"""
    out = {}
    for body in re.findall(r"enum\s*\{(.*?)\};", text, flags=re.S):
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        val = -1
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            m = re.match(r"(\w+)(?:\s*=\s*(\d+))?$", item)
            if not m:
                break
            val = int(m.group(2)) if m.group(2) is not None else val + 1
            if m.group(1).startswith(prefix):
                out[m.group(1)] = val
    return out


def test_header_declares_the_ten_entry_points_and_their_field_enums():
    text = open(HEADER).read()
    for m in MODULES:
        sig = re.search(r"ZH_API int (zh_%s_paint_spans)\((.*?)\);" % m, text, flags=re.S)
        assert sig, m
        args = " ".join(sig.group(2).split())
        assert re.sub(r"/\*.*?\*/", "", args).replace("  ", " ") == (
            "zh_%s *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps, const zh_%s_params *params, "
            "const zh_script_span_param *span_params , const zh_script_span_table *table, uint32_t flags" % (m, m)), args
        vals = _enum_values(text, "ZH_%s_SPAN_" % m.upper())
        names = FIELDS[m]
        for i, f in enumerate(names):
            assert vals["ZH_%s_SPAN_%s" % (m.upper(), f)] == i, (m, f, vals)
        assert vals["ZH_%s_SPAN_FIELDS" % m.upper()] == len(names), (m, vals)


def test_ctypes_mirror_has_the_signatures_and_field_enums():
    from zang_amd import abi
    for m in MODULES:
        res, args = abi.SIGNATURES["zh_%s_paint_spans" % m]
        assert res is C.c_int and len(args) == 9
        assert args[6] is C.POINTER(abi.ScriptSpanParam) and args[7] is C.POINTER(abi.ScriptSpanTable)
        for i, f in enumerate(FIELDS[m]):
            assert getattr(abi, "%s_SPAN_%s" % (m.upper(), f)) == i
        assert getattr(abi, "%s_SPAN_FIELDS" % m.upper()) == len(FIELDS[m])


def test_python_classes_list_the_fields_in_the_c_order():
    from zang_amd import modules as mod
    classes = {"sineosc": mod.SineOsc, "pulseosc": mod.PulseOsc, "trisawosc": mod.TriSawOsc, "noise": mod.Noise, "envelope": mod.Envelope,
               "gate": mod.Gate, "filter": mod.Filter, "sampler": mod.Sampler, "decimator": mod.Decimator, "distortion": mod.Distortion}
    for m, cls in classes.items():
        assert [n.upper() for n, _ in cls._span_fields] == FIELDS[m], m


def test_zig_binding_declares_span_params_as_many_pointers():
    text = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    for m in MODULES:
        line = re.search(r"pub extern fn zh_%s_paint_spans\((.*?)\) c_int;" % m, text)
        assert line, m
        assert "span_params: ?[*]const ScriptSpanParam" in line.group(1), line.group(1)
        assert "table: ?*const ScriptSpanTable" in line.group(1), line.group(1)
        assert "pub const %s_SPAN_FIELDS: u32 = %d;" % (m.upper(), len(FIELDS[m])) in text


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


def test_paint_spans_builds_the_ctypes_arguments_without_a_device():
    """Filter.paint_spans with a table whose `type` and `cutoff` vary per sub-span: one zh_filter_paint_spans call with the span
    and flags, the table's arrays, span_params in the C field order (type: u only, cutoff: f only, res: none)."""
    from zang_amd import abi, modules as mod, zang
    m = object.__new__(mod.Filter)
    m.lib, m.handle, m.ctx, m.n_voices = _FakeLib(), C.c_void_p(1234), _FakeCtx(), 4
    V = 4
    types = np.array([[1, 2, 3, 4], [0, 5, 1, 1]], np.uint32)
    cut = np.full((2, V), 0.25, np.float32)
    table = m.span_table(np.array([1, 2, 0, 1]), np.array([[0, 0, 0, 10], [0, 512, 0, 0]]), np.array([[1024, 512, 0, 20], [0, 1024, 0, 0]]),
                         np.array([[1, 0, 0, 1], [0, 1, 0, 0]]), {"type": (None, types), "cutoff": (cut, None)})
    inp = abi.Buf(0x1000, V, 1024, V, 0)
    params = mod.Filter.Params(inp, 1, zang.constant(0.5), zang.constant(0.1))
    out = abi.Buf(0x2000, V, 1024, V, 0)
    rc = m._paint_spans(zang.Span(16, 1000), [out], None, params, table, abi.PAINT_ZERO_FIRST)
    assert rc == 0
    (args,) = m.lib.fns["zh_filter_paint_spans"].calls
    handle, s, e, outs, temps, cp, sp, tb, flags = args
    assert (s, e, flags) == (16, 1000, abi.PAINT_ZERO_FIRST) and temps is None and handle.value == 1234
    assert outs[0].ptr == 0x2000 and outs[0].voices == V
    cp = cp._obj
    assert cp.type == 1 and cp.input.ptr == 0x1000 and abs(cp.cutoff.constant.value - 0.5) < 1e-7
    tb = tb._obj
    assert tb.max_spans == 2
    assert np.ctypeslib.as_array(C.cast(tb.count, C.POINTER(C.c_uint32)), (V,)).tolist() == [1, 2, 0, 1]
    assert np.ctypeslib.as_array(C.cast(tb.end, C.POINTER(C.c_uint32)), (2, V)).tolist() == [[1024, 512, 0, 20], [0, 1024, 0, 0]]
    assert np.ctypeslib.as_array(C.cast(tb.note_id_changed, C.POINTER(C.c_uint8)), (2, V)).tolist() == [[1, 0, 0, 1], [0, 1, 0, 0]]
    assert sp[abi.FILTER_SPAN_TYPE].f is None and sp[abi.FILTER_SPAN_TYPE].u is not None
    assert np.ctypeslib.as_array(C.cast(sp[abi.FILTER_SPAN_TYPE].u, C.POINTER(C.c_uint32)), (2, V)).tolist() == types.tolist()
    assert sp[abi.FILTER_SPAN_CUTOFF].f is not None and sp[abi.FILTER_SPAN_CUTOFF].u is None
    assert sp[abi.FILTER_SPAN_RES].f is None and sp[abi.FILTER_SPAN_RES].u is None


def test_span_table_from_a_poly_schedule_layout():
    """span_table() takes the [span][voice] layout zh_poly_voice_schedule fills; fields outside the module are refused."""
    import pytest
    from zang_amd import modules as mod
    t = mod.Gate.span_table(np.ones(3), np.zeros((1, 3)), np.full((1, 3), 64), np.zeros((1, 3)), {"note_on": (None, np.ones((1, 3)))})
    assert t.max_spans == 1 and t.n_voices == 3 and t.arrays["note_on"][1].dtype == np.uint32
    with pytest.raises(KeyError):
        mod.Gate.span_table(np.ones(3), np.zeros((1, 3)), np.full((1, 3), 64), np.zeros((1, 3)), {"freq": (np.ones((1, 3)), None)})
