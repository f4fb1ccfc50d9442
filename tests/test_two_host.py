"""CPU: the host side of the two-source player without a device: TwoKeys (zang_amd/two.py) against the model's keyEvent
(tests/two_reference.py), event by event; the records and the merge stage's source descriptors; the surface -- header, ctypes
mirror and struct sizes agree."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import two_reference as tr
from tests.hostprog import c_ints, mirror_layout

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_FREQS = [f32(2.0 ** (k / 12.0)) for k in range(-12, 13)]


def _rel(key):
    return REL_FREQS[3 * key + 2]


def test_two_keys_is_key_event(oracle):
    """the key rule alone: TwoKeys against the model's keyEvent, event by event"""
    from zang_amd import two
    keys, m = two.TwoKeys(880.0), tr.MainModule(oracle, 880.0)
    first = keys.first()
    m._first()
    assert [(0, i, (f, on)) for i, f, on in first] == [m.iq0.items[0], m.iq1.items[0]] and first[0][1] == f32(440.0) and first[1][1] == f32(0.5)
    for kind, key, down in [("k", 1, True), ("k", 2, True), ("k", 1, False), ("k", 2, False), ("k", 2, False), ("n", 0, True), ("n", 8, True),
                            ("n", 0, False), ("n", 8, False), ("n", 4, True), ("k", 3, False)]:
        before = (len(m.iq0.items), len(m.iq1.items))
        if kind == "k":
            ev = keys.note_key(key, down, _rel(key))
            m.key_event(key, down, 5, rel_freq=_rel(key))
            new = m.iq0.items[before[0]:]
        else:
            ev = keys.number_key(key, down)
            m.key_event(key, down, 5, number=key)
            new = m.iq1.items[before[1]:]
        assert (ev is None) == (not new), (kind, key, down)
        if ev is not None:
            assert (5, ev[0], (ev[1], ev[2])) == new[0] and np.asarray(ev[1]).dtype == f32, (kind, key, down)
    assert keys.number_key(8, True)[1] == f32(1.0) and keys.number_key(0, True)[1] == f32(0.5)
    with pytest.raises(ValueError):
        keys.number_key(9, True)


def test_records_and_source_descriptors():
    from zang_amd import abi, two
    assert two.FREQ_PARAMS.names == ("freq", "note_on", "on") and two.COLOR_PARAMS.names == ("color", "note_on", "on")
    assert two.FREQ_PARAMS.itemsize == two.COLOR_PARAMS.itemsize == 12 and two.FREQ_PARAMS.fields["on"][1] == 8
    d = two._source([("freq", "f"), ("note_on_a", "u")], "note_on_a")
    assert (d.n_fields, d.on_field, bytes(d.kinds)) == (2, 1, b"fu\0\0")
    assert two._source([("x", "u")], "missing").on_field == 1           # an unknown note-on name: out of range, the library refuses it
    assert two.MAX_SPANS == 2 * two.SOURCE_SPANS - 1


def test_struct_sizes_match_gcc(tmp_path):
    from zang_amd import abi
    names = {"zh_span_merge_source": abi.SpanMergeSource, "zh_dual_patch": abi.DualPatch, "zh_dual_params": abi.DualParams, "zh_dual_state": abi.DualState}
    own, = c_ints(["ZH_SPAN_MERGE_OWN_FIELDS * 100 + ZH_SPAN_MERGE_NIC_B * 10 + ZH_SPAN_MERGE_NIC_A"])
    assert own == 321 == abi.SPAN_MERGE_OWN_FIELDS * 100 + abi.SPAN_MERGE_NIC_B * 10 + abi.SPAN_MERGE_NIC_A
    _, seen = mirror_layout(names)
    assert seen == 4 + 3 + 4 + 6 + 2


def test_null_handles_are_refused():
    from zang_amd import abi
    lib = abi.load()
    h = C.c_void_p()
    src = abi.SpanMergeSource(1, 0, (C.c_uint8 * 4)(ord("u"), 0, 0, 0))
    assert lib.zh_span_merge_create(None, 4, C.byref(src), C.byref(src), C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_destroy(None) == abi.ZH_ERR_INVALID and lib.zh_span_merge_reserve(None, 4) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_schedule(None, 256, 4, None, None, None, None) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_script_table(None, 4, None) == abi.ZH_ERR_INVALID and lib.zh_span_merge_span_param(None, 0, None) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_overflows(None, None) == abi.ZH_ERR_INVALID
    assert lib.zh_dual_create(None, 4, C.byref(h)) == abi.ZH_ERR_INVALID and lib.zh_dual_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_dual_get_state(None, None) == abi.ZH_ERR_INVALID and lib.zh_dual_set_state(None, None) == abi.ZH_ERR_INVALID
    p = abi.DualParams()
    assert lib.zh_dual_paint(None, 0, 0, None, None, abi.Bool(), C.byref(p), 0) == abi.ZH_ERR_INVALID
    assert lib.zh_dual_paint_spans(None, 0, 0, None, None, C.byref(p), None, None, 0) == abi.ZH_ERR_INVALID
    patch = abi.DualPatch()
    assert lib.zh_dual_patch_default(C.byref(patch)) == 0 and lib.zh_dual_patch_default(None) == abi.ZH_ERR_INVALID
    assert tuple(f32(x) for x in (patch.attack, patch.decay, patch.release, patch.sustain_volume)) == tuple(f32(x) for x in tr.DEFAULT_PATCH)
