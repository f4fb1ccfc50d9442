"""GPU: the fused FM voice (zh_fm_paint, k_fm in csrc/fm.hip) against tests/fm_reference.py -- the np.float32 restatement of
examples/example_fmsynth.zig:22-356 that tests/test_fm_reference.py pins to the oracle -- over the corpus of tests/fm_cases.py:
130 voices (two full waves and a 2-lane tail) in 26 instruments of 5, 1,024 frames as the chain (0,200) (200,777) (777,1024)
(0,1024).  Every comparison is bit for bit; the reference is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import fm_cases as fc
from tests import fm_reference as fr
from tests.util import assert_bitexact, dev, from_image, to_image

pytestmark = pytest.mark.gpu
V, F, SR, GROUP, NI = fc.V, fc.F, fc.SR, fc.GROUP, fc.NI


def _instrument(ctx, group=GROUP, patches=None, n=V):
    from zang_amd import modules as mod
    m = mod.FMInstrument(n, ctx, group=group)
    m.set_patches(np.array(fc.patches() if patches is None else patches, np.uint32))
    return m


def _params(k, trem=None, vib=None, freq=None):
    """the chain's paint k: per-voice freq / note_on / note_id_changed arrays on the device"""
    from zang_amd import modules as mod
    x = fc.inputs()
    p = mod.FMInstrument.Params(SR, to_image(x["trem"]) if trem is None else trem, to_image(x["vib"]) if vib is None else vib,
                                dev(x["freq"] if freq is None else freq), dev(x["on"][k].astype(np.uint8)))
    return p, dev(x["nic"][k].astype(np.uint8))


def _state(m):
    """zh_fm_state [V] -> fm_reference.STATE_DTYPE [V][2] (the same 32 bytes per operator)"""
    return np.frombuffer(m.state().tobytes(), fr.STATE_DTYPE).reshape(m.n_voices, 2)


def _assert_state(m, want, what):
    got = _state(m)
    for name in fr.STATE_DTYPE.names:
        assert_bitexact(got[name], want[name], f"{what}: state.{name}")


def _chain(ctx, m, img, zero_first=False, upto=len(fc.CHAIN), first=0, split=False):
    from zang_amd import zang
    for k in range(first, upto):
        p, nic = _params(k)
        m.paint(zang.Span(*fc.CHAIN[k]), [img], None, nic, p, zero_first=zero_first, split=split)
        yield k


def test_chain_on_a_live_image_and_the_state_after_every_paint(ctx):
    x, ref = fc.inputs(), fc.reference()
    want = fc.expected_images(x["live"])
    m = _instrument(ctx)
    img = to_image(x["live"])
    for k in _chain(ctx, m, img):
        ctx.sync()
        assert_bitexact(from_image(img), want[k], f"paint {k}")
        _assert_state(m, ref["paints"][k]["state"], f"paint {k}")
    assert any("k_fm" in name and "spans" not in name for name in ctx.last_form()), ctx.last_form()
    m.close()


def test_zero_first_writes_the_span_from_zero_and_nothing_else(ctx):
    x, ref = fc.inputs(), fc.reference()
    m = _instrument(ctx)
    img = to_image(x["live"])
    want = x["live"].copy()
    for k in _chain(ctx, m, img, zero_first=True):
        s, e = fc.CHAIN[k]
        want[:, s:e] = 0.0
        p = ref["paints"][k]
        fr.add_into(want, np.arange(V), s, e, p["m"], p["c"], p["add_m"])
        ctx.sync()
        assert_bitexact(from_image(img), want, f"paint {k}")
    _assert_state(m, ref["paints"][-1]["state"], "after the chain")
    m.close()


def test_strided_views_of_output_and_lfo_images(ctx):
    """the output a column range of a wider image at an odd offset, the LFO images column ranges of one shared image"""
    import torch
    from zang_amd import modules as mod, zang
    x = fc.inputs()
    want = fc.expected_images(x["live"])
    wide = torch.full((F, V + 37), 7.0, dtype=torch.float32, device=ctx.device)
    img = wide[:, 3:3 + V]
    img.copy_(to_image(x["live"]))
    lfo = torch.full((F, 2 * NI + 5), -3.0, dtype=torch.float32, device=ctx.device)
    trem, vib = lfo[:, 1:1 + NI], lfo[:, 2 + NI:2 + 2 * NI]
    trem.copy_(to_image(x["trem"])); vib.copy_(to_image(x["vib"]))
    m = _instrument(ctx)
    for k in range(len(fc.CHAIN)):
        p, nic = _params(k, trem, vib)
        m.paint(zang.Span(*fc.CHAIN[k]), [img], None, nic, p)
    ctx.sync()
    assert_bitexact(from_image(img), want[-1], "the view")
    rest = wide.cpu().numpy()
    assert (rest[:, :3] == 7.0).all() and (rest[:, 3 + V:] == 7.0).all(), "columns outside the view were written"
    _assert_state(m, fc.reference()["paints"][-1]["state"], "after the chain")
    m.close()


def test_state_round_trip_mid_chain(ctx):
    x, ref = fc.inputs(), fc.reference()
    want = fc.expected_images(x["live"])
    a = _instrument(ctx)
    img = to_image(x["live"])
    for _ in _chain(ctx, a, img, upto=2):
        pass
    st = a.state()
    b = _instrument(ctx)
    b.set_state(st)
    assert b.state().tobytes() == st.tobytes()
    for _ in _chain(ctx, b, img, first=2):
        pass
    ctx.sync()
    assert_bitexact(from_image(img), want[-1], "a fresh instrument continued from the state")
    _assert_state(b, ref["paints"][-1]["state"], "after the chain")
    a.close(); b.close()


def test_group_of_one_with_repeated_columns_equals_groups_of_five(ctx):
    from zang_amd import zang
    x = fc.inputs()
    want = fc.expected_images(x["live"])
    per_voice = np.repeat(np.array(fc.patches(), np.uint32), GROUP, axis=0)
    m = _instrument(ctx, group=1, patches=per_voice)
    assert m.n_instruments == V
    trem, vib = to_image(np.repeat(x["trem"], GROUP, axis=0)), to_image(np.repeat(x["vib"], GROUP, axis=0))
    img = to_image(x["live"])
    for k in range(len(fc.CHAIN)):
        p, nic = _params(k, trem, vib)
        m.paint(zang.Span(*fc.CHAIN[k]), [img], None, nic, p)
    ctx.sync()
    assert_bitexact(from_image(img), want[-1], "group = 1")
    _assert_state(m, fc.reference()["paints"][-1]["state"], "group = 1")
    m.close()


def test_one_patch_for_every_instrument_and_the_default(ctx):
    """n_patches == 1 reaches every instrument; a new instrument is on the default patch (:376-397)"""
    from zang_amd import zang
    x = fc.inputs()
    ref = fr.FMRef(V, GROUP)                                             # the default patch
    p, nic = _params(0)
    want = x["live"].copy()
    ref.paint_into(want, 0, 200, x["nic"][0], SR, x["trem"], x["vib"], x["freq"], x["on"][0])
    from zang_amd import modules as mod
    fresh = mod.FMInstrument(V, ctx, group=GROUP)
    one = _instrument(ctx, patches=[fc.patches()[9]])
    one.set_patches(np.array([fr.DEFAULT_PATCH], np.uint32))
    for m in (fresh, one):
        img = to_image(x["live"])
        m.paint(zang.Span(0, 200), [img], None, nic, p)
        ctx.sync()
        assert_bitexact(from_image(img), want, "the default patch")
        m.close()


def test_split_operators(ctx):
    """on a zeroed image the columns are m and c; (live + m) + c formed on the host is the unsplit paint onto live"""
    x, ref = fc.inputs(), fc.reference()
    want_unsplit = fc.expected_images(x["live"])
    m = _instrument(ctx)
    img = ctx.image(F, 2 * V, fill=5.0)
    live = x["live"].copy()
    for k in _chain(ctx, m, img, zero_first=True, split=True):
        s, e = fc.CHAIN[k]
        p = ref["paints"][k]
        ctx.sync()
        got = from_image(img)
        assert_bitexact(got[0::2, s:e], np.where(p["add_m"][:, None], np.float32(0) + p["m"], np.float32(0)).astype(np.float32), f"paint {k}: m")
        assert_bitexact(got[1::2, s:e], (np.float32(0) + p["c"]).astype(np.float32), f"paint {k}: c")
        if k < 3:
            assert (got[:, e:] == 5.0).all(), "frames after the span were written"
        mm, cc = got[0::2, s:e], got[1::2, s:e]
        live[:, s:e] = np.where(p["add_m"][:, None], live[:, s:e] + mm, live[:, s:e]) + cc
        assert_bitexact(live, want_unsplit[k], f"paint {k}: (live + m) + c")
    _assert_state(m, ref["paints"][-1]["state"], "split")
    # without ZERO_FIRST the split columns are added to
    m2 = _instrument(ctx)
    base = np.random.default_rng(3).uniform(-1, 1, (2 * V, F)).astype(np.float32)
    img2 = to_image(base)
    for _ in _chain(ctx, m2, img2, upto=1, split=True):
        pass
    ctx.sync()
    p = ref["paints"][0]
    want = base.copy()
    want[:, 0:200] = fr.split_image(base[:, 0:200], p["m"], p["c"], np.ones((V, 200), bool), p["add_m"])
    assert_bitexact(from_image(img2), want, "split, added")
    m.close(); m2.close()


def test_set_patches_refuses_a_bad_value_and_changes_nothing(ctx):
    from zang_amd import abi, zang
    x = fc.inputs()
    want = fc.expected_images(x["live"])
    m = _instrument(ctx)
    L = ctx.lib
    good = np.array(fc.patches(), np.uint32)
    for k, n in enumerate(fr.NUM_VALUES):
        bad = good.copy()
        bad[:, :] = np.array(fr.DEFAULT_PATCH, np.uint32)               # every other patch would change ...
        bad[NI - 1, k] = n                                                # ... if the last one's bad value were found too late
        assert L.zh_fm_set_patches(m.handle, bad.ctypes.data, NI) == abi.ZH_ERR_INVALID, k
    assert L.zh_fm_set_patches(m.handle, good.ctypes.data, NI - 1) == abi.ZH_ERR_INVALID
    assert L.zh_fm_set_patches(m.handle, good.ctypes.data, 0) == abi.ZH_ERR_INVALID
    assert L.zh_fm_set_patches(m.handle, None, NI) == abi.ZH_ERR_INVALID
    assert L.zh_fm_set_patches(None, good.ctypes.data, NI) == abi.ZH_ERR_INVALID
    img = to_image(x["live"])
    for _ in _chain(ctx, m, img):
        pass
    ctx.sync()
    assert_bitexact(from_image(img), want[-1], "after the refused set_patches calls")
    m.close()


def test_refusals(ctx):
    import torch
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_bool, as_buf, as_f32
    L = ctx.lib
    bad, unsupported = abi.ZH_ERR_INVALID, abi.ZH_ERR_UNSUPPORTED
    h = C.c_void_p()
    assert L.zh_fm_create(None, V, GROUP, C.byref(h)) == bad and L.zh_fm_create(ctx.handle, V, GROUP, None) == bad
    assert L.zh_fm_create(ctx.handle, V, 0, C.byref(h)) == bad
    assert L.zh_fm_destroy(None) == bad and L.zh_fm_get_state(None, None) == bad and L.zh_fm_set_state(None, None) == bad
    m = mod.FMInstrument(V, ctx, group=GROUP)
    assert L.zh_fm_get_state(m.handle, None) == bad and L.zh_fm_set_state(m.handle, None) == bad
    out, out2 = ctx.image(F, V, fill=0.0), ctx.image(F, 2 * V, fill=0.0)
    lfo = ctx.image(F, NI, fill=0.0)
    nic = as_bool(False)

    def paint(handle=m.handle, s=0, e=F, o=out, trem=lfo, vib=lfo, flags=0, params=True, outputs=True):
        p = abi.FMParams(SR, 0, as_buf(trem), as_buf(vib), as_f32(440.0), as_bool(True))
        bufs = (abi.Buf * 1)(as_buf(o))
        return L.zh_fm_paint(handle, s, e, bufs if outputs else None, None, nic, C.byref(p) if params else None, flags)
    assert paint() == abi.ZH_OK
    assert paint(handle=None) == bad and paint(params=False) == bad and paint(outputs=False) == bad
    assert paint(s=5, e=4) == bad and paint(e=F + 1) == bad
    assert paint(o=out[:, :V - 1]) == bad                                 # too few columns
    assert paint(flags=abi.FM_SPLIT_OPERATORS) == bad                     # split needs 2 * n_voices columns
    assert paint(o=out2, flags=abi.FM_SPLIT_OPERATORS) == abi.ZH_OK
    assert paint(trem=lfo[:, :NI - 1]) == bad and paint(vib=lfo[:, :NI - 1]) == bad     # one LFO column per instrument
    assert paint(trem=lfo[:F - 1]) == bad and paint(vib=lfo[:F - 1]) == bad             # the span outside an LFO image
    null = abi.Buf(None, V, F, V, 0)
    assert paint(o=null) == bad and paint(trem=abi.Buf(None, NI, F, NI, 0)) == bad
    assert paint(flags=abi.PAINT_TOLERANT) == unsupported                 # exact forms only
    assert paint(s=7, e=7) == abi.ZH_OK                                   # an empty span is a paint call like any other

    # the span paint: the same, and a bad table
    from zang_amd.spans import SpanTable
    tb = SpanTable([[(0, F, 440.0, True, True)]] * V, ctx.device)

    def spans(handle=m.handle, s=0, e=F, o=out, trem=lfo, vib=lfo, table=tb.c, flags=0, outputs=True):
        bufs = (abi.Buf * 1)(as_buf(o))
        return L.zh_fm_paint_spans(handle, s, e, bufs if outputs else None, None, SR, as_buf(trem), as_buf(vib),
                                   C.byref(table) if table is not None else None, flags)
    assert spans() == abi.ZH_OK
    assert spans(handle=None) == bad and spans(outputs=False) == bad and spans(table=None) == bad
    assert spans(s=5, e=4) == bad and spans(e=F + 1) == bad and spans(o=out[:, :V - 1]) == bad
    assert spans(flags=abi.FM_SPLIT_OPERATORS) == bad and spans(o=out2, flags=abi.FM_SPLIT_OPERATORS) == abi.ZH_OK
    assert spans(trem=lfo[:, :NI - 1]) == bad and spans(vib=lfo[:F - 1]) == bad
    assert spans(flags=abi.PAINT_TOLERANT) == unsupported
    for field in ("count", "start", "end", "freq", "note_on", "note_id_changed"):
        t2 = abi.SpanTable.from_buffer_copy(tb.c)
        setattr(t2, field, None)
        assert spans(table=t2) == bad, field
    t2 = abi.SpanTable.from_buffer_copy(tb.c)
    t2.max_spans = 0
    assert spans(table=t2) == bad
    ctx.sync()
    m.close()


def test_set_patches_is_refused_while_a_capture_records_and_a_paint_is_recorded(ctx):
    import torch
    import zang_amd
    from zang_amd import abi, modules as mod, zang
    x, ref = fc.inputs(), fc.reference()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        m = mod.FMInstrument(V, c2, group=GROUP)
        good = np.array(fc.patches(), np.uint32)
        m.set_patches(good)
        img = to_image(x["live"])
        p, nic = _params(0)
    c2.sync()
    rcs = []

    def body():
        rcs.append(c2.lib.zh_fm_set_patches(m.handle, good.ctypes.data, NI))
        m.paint(zang.Span(*fc.CHAIN[0]), [img], None, nic, p)
    g = c2.capture(body)
    assert rcs == [abi.ZH_ERR_UNSUPPORTED]
    assert any("k_fm" in k for k, _ in g.kernels()), g.kernels()
    g.launch()
    c2.sync()
    assert_bitexact(from_image(img), fc.expected_images(x["live"])[0], "the replayed paint")
    _assert_state(m, ref["paints"][0]["state"], "the replayed paint")
    g.close()
    m.close()
    c2.close()


def test_no_voices(ctx):
    from zang_amd import modules as mod, zang
    m = mod.FMInstrument(0, ctx, group=3)
    assert m.n_instruments == 0 and len(m.state()) == 0
    m.close()
