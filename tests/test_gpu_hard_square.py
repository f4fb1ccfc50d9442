"""GPU: the HardSquare voice -- zh_hard_square_paint[_spans] (k_hard_square_spans) -- against the oracle's zo_hard_square_paint plus
zo_add_scalar_into, per voice and per sub-span (tests/arp_reference.py hard_square_paint under tests/lead_reference.py's Trigger
loop).  Everything on bits: the uint32 views of both output images and the PulseOsc's cnt after every buffer; any NaN equals any
NaN (by position)."""
import ctypes as C

import numpy as np
import pytest

from tests import hard_square_cases as hq
from tests import hostile_cases as hc
from tests import lead_cases as lc
from tests import lead_reference as lr
from tests import util

pytestmark = pytest.mark.gpu


def _table(m, tb, names=lr.FIELDS):
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], lc.span_values(tb, names) if names else None)


def _check(m, out, sync, ref, rsync, vs, what):
    got = util.from_image(out)
    assert hc.same_f32(got, ref), (what, hc.first_difference(got, ref))
    if sync is not None:
        gs = util.from_image(sync)
        assert hc.same_f32(gs, rsync), (what + " sync", hc.first_difference(gs, rsync))
    assert np.array_equal(m.state()["osc"]["cnt"], hq.cnts(vs)), what + " state"


@pytest.mark.parametrize("V", hq.VOICES)
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
@pytest.mark.parametrize("with_sync", [True, False], ids=["sync", "no_sync"])
def test_span_paint_equals_the_oracle_per_sub_span(ctx, oracle, V, zero_first, with_sync):
    """Two consecutive buffers with carried state, both fields from span arrays: the FIXED shapes in voices 0-4 (adjacent, an empty
    one between, overlapping -- the list ends there --, empty at either edge, none at all), note-offs whose multiply-add still
    runs, -0.0 planted in the bases; rows outside [3, 250) keep their bits"""
    from zang_amd import modules as mod, zang
    m = mod.HardSquare(V, ctx)
    vs = hq.voices(oracle, V)
    for b in range(2):
        tb = lc.tables(V, 1000 * V + b, note_on_first=b == 0)
        base, sbase = lc.base_image(V, 77 + V + b), lc.base_image(V, 177 + V + b)
        ref, rsync = base.copy(), (sbase.copy() if with_sync else None)
        hq.reference_spans(oracle, vs, tb, ref, rsync, zero_first)
        out, sync = util.to_image(base), (util.to_image(sbase) if with_sync else None)
        m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, m.Params(hq.SR), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_hard_square_spans"], ctx.last_form()
        _check(m, out, sync, ref, rsync, vs, f"V={V} buffer {b}")
        assert not lc.same_bits(ref, base)
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_plain_paint_equals_the_oracle_and_the_span_form(ctx, oracle, V):
    """zh_hard_square_paint: V voices with their own freq and note_on painting the span three times (ADD, ZERO_FIRST, ADD), the
    frequency image in the first two, with carried state == the oracle == the span form over one full sub-span per voice"""
    from zang_amd import modules as mod, zang
    S, E = lc.SPAN
    ms = [mod.HardSquare(V, ctx) for _ in range(2)]
    vs = hq.voices(oracle, V)
    for b in range(3):
        tb = lc.one_span_tables(V, 77 * V + b)
        base, sbase = lc.base_image(V, 31 + V + b), lc.base_image(V, 131 + V + b)
        ref, rsync = base.copy(), (sbase.copy() if b < 2 else None)
        hq.reference_spans(oracle, vs, tb, ref, rsync, b == 1)
        outs = [(util.to_image(base), util.to_image(sbase) if b < 2 else None) for _ in range(2)]
        params = ms[0].Params(hq.SR, util.dev(tb["freq"][0]), util.dev(tb["note_on"][0].astype(np.uint8)))
        ms[0].paint(zang.Span(S, E), list(outs[0]), [], False, params, zero_first=b == 1)
        ms[1].paint_spans(zang.Span(S, E), list(outs[1]), None, ms[1].Params(hq.SR), _table(ms[1], tb), zero_first=b == 1)
        ctx.sync()
        for i, what in enumerate(("plain", "one sub-span")):
            _check(ms[i], outs[i][0], outs[i][1], ref, rsync, vs, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


@pytest.mark.parametrize("how", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, how):
    from zang_amd import modules as mod, zang
    V = 65
    tb = lc.tables(V, 4242)
    m = mod.HardSquare(V, ctx)
    vs = hq.voices(oracle, V)
    rng = np.random.default_rng(5)
    if how == "broadcast":
        dflt, params, names = {"freq": np.float32(330.0), "note_on": 1}, m.Params(hq.SR, 330.0, True), ()
    else:
        dflt = {"freq": rng.uniform(110.0, 880.0, V).astype(np.float32), "note_on": (np.arange(V) % 3 != 0).astype(np.uint32)}
        params = m.Params(hq.SR, util.dev(dflt["freq"]), util.dev(dflt["note_on"].astype(np.uint8)))
        names = () if how == "per_voice" else ("freq",)
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base, sbase = lc.base_image(V, 3), lc.base_image(V, 4)
    ref, rsync = base.copy(), sbase.copy()
    hq.reference_spans(oracle, vs, lean, ref, rsync, False, dflt=dflt)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, params, _table(m, tb, names))
    ctx.sync()
    _check(m, out, sync, ref, rsync, vs, how)
    m.close()


def test_a_frequency_out_of_range_paints_nothing_and_the_adds_still_happen(ctx, oracle):
    """freq either side of sample_rate / 8 = 6000 and below 0 over images holding -0.0: where the PulseOsc paints nothing
    out0 += 0 * gate still runs, so -0.0 becomes +0.0 inside the sub-span and stays outside; cnt does not move"""
    from zang_amd import modules as mod, zang
    V = 65
    tb = lc.tables(V, 606)
    rng = np.random.default_rng(9)
    tb["freq"][:] = rng.choice(np.array([5900.0, 5999.0, 6000.0, 6001.0, 6100.0, -1.0, -220.0, 440.0], np.float32), tb["freq"].shape)
    tb["count"][1], tb["start"][0, 1], tb["end"][0, 1], tb["freq"][0, 1], tb["note_on"][0, 1] = 1, 180, 230, 7000.0, 1
    m = mod.HardSquare(V, ctx)
    vs = hq.voices(oracle, V)
    base, sbase = lc.base_image(V, 12), lc.base_image(V, 13)
    ref, rsync = base.copy(), sbase.copy()
    hq.reference_spans(oracle, vs, tb, ref, rsync, False)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, m.Params(hq.SR), _table(m, tb))
    ctx.sync()
    _check(m, out, sync, ref, rsync, vs, "out of range")
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (bits(ref[1, 200:230]) == 0).all() and (bits(ref[1, 230:250]) == 0x80000000).all() and vs[1].cnt == 0
    m.close()


def test_hostile_freq_in_the_last_sub_span(ctx, oracle):
    from zang_amd import modules as mod, zang
    V, tb = lc.hostile_freq_tables()
    m = mod.HardSquare(V, ctx)
    vs = hq.voices(oracle, V)
    base, sbase = lc.base_image(V, 90), lc.base_image(V, 91)
    ref, rsync = base.copy(), sbase.copy()
    hq.reference_spans(oracle, vs, tb, ref, rsync, False)
    share = lc.worst_row_nan_share(ref, rsync)
    print("hard_square hostile freq: worst NaN share of a voice", share)
    assert 0.0 < share <= hq.NAN_CAP                                 # the oracle alone (tests/test_hard_square_reference.py too)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, m.Params(hq.SR), _table(m, tb))
    ctx.sync()
    _check(m, out, sync, ref, rsync, vs, "hostile freq")
    m.close()


@pytest.mark.parametrize("sample_rate", lc.HOSTILE_SR, ids=["zero", "negative", "nan", "inf", "denormal"])
def test_hostile_sample_rates_equal_the_oracle(ctx, oracle, sample_rate):
    """a clean plain paint over [3, 200), then one over [200, 250) with the hostile rate; 65 voices with their own freq and note_on"""
    from zang_amd import modules as mod, zang
    V = 65
    S, E = lc.SPAN
    rng = np.random.default_rng(17)
    m = mod.HardSquare(V, ctx)
    vs = hq.voices(oracle, V)
    base, sbase = lc.base_image(V, 900), lc.base_image(V, 910)
    ref, rsync = base.copy(), sbase.copy()
    out, sync = util.to_image(base), util.to_image(sbase)
    for b, (s, e, sr) in enumerate(((S, lc.HOSTILE_FROM, hq.SR), (lc.HOSTILE_FROM, E, sample_rate))):
        freq = rng.uniform(110.0, 880.0, V).astype(np.float32)
        on = np.ones(V, np.uint8) if b == 0 else (np.arange(V) % 3 != 0).astype(np.uint8)
        hq.reference_plain(oracle, vs, s, e, ref, rsync, sr, freq, on)
        m.paint(zang.Span(s, e), [out, sync], [], False, m.Params(sr, util.dev(freq), util.dev(on)))
    ctx.sync()
    share = lc.worst_row_nan_share(ref, rsync)
    print("hard_square sample_rate", sample_rate, "worst NaN share of a voice", share)
    assert share <= hq.NAN_CAP
    _check(m, out, sync, ref, rsync, vs, f"sample_rate {sample_rate}")
    m.close()


def test_state_round_trip(ctx, oracle):
    from zang_amd import modules as mod, zang
    V = 3
    m = mod.HardSquare(V, ctx)
    st = m.state()
    assert (st["osc"]["cnt"] == 0).all()                             # create == init()
    st["osc"]["cnt"][:] = (1, 0x80000000, 0xfffffff0)
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    vs = hq.voices(oracle, V)
    for v in range(V):
        vs[v].st.osc.cnt = int(st["osc"]["cnt"][v])
    S, E = lc.SPAN
    base, sbase = lc.base_image(V, 8), lc.base_image(V, 9)
    ref, rsync = base.copy(), sbase.copy()
    hq.reference_plain(oracle, vs, S, E, ref, rsync, hq.SR, 220.0, True)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint(zang.Span(S, E), [out, sync], [], False, m.Params(hq.SR, 220.0, True))
    ctx.sync()
    _check(m, out, sync, ref, rsync, vs, "from a set state")
    m.close()


def test_refusals(ctx):
    import torch
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf
    V = 8
    tb = lc.tables(V, 1)
    m = mod.HardSquare(V, ctx)
    paint, paint_spans = ctx.lib.zh_hard_square_paint, ctx.lib.zh_hard_square_paint_spans
    out, sync = ctx.image(lc.ROWS, V, fill=0.25), ctx.image(lc.ROWS, V, fill=0.5)
    before, sbefore = out.clone(), sync.clone()
    state = m.state().tobytes()
    span = zang.Span(*lc.SPAN)
    good = m.Params(hq.SR)
    assert m._paint_spans(span, [out, sync], None, good, _table(m, tb), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_spans(span, [out[:50], sync], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID      # too few rows
    assert m._paint_spans(span, [out[:, :V - 1], sync], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID  # too few voices
    assert m._paint_spans(span, [out, sync[:50]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID      # the second output too small
    wide, marker = ctx.image(lc.ROWS, 2 * V, fill=0.5), ctx.last_form()    # outputs[1] shares a float with outputs[0]: refused, no launch
    assert m._paint_spans(span, [out, out], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID                  # the same image
    assert m._paint_spans(span, [wide[:, :V], wide[:, V - 1:2 * V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID   # one column in common
    assert ctx.last_form() == marker
    with pytest.raises(abi.ZangHipError):
        m.paint(span, [out[:50]], [], False, good)
    outs = (abi.Buf * 2)(as_buf(out), as_buf(sync))
    null0 = (abi.Buf * 2)(abi.Buf(), as_buf(sync))
    ctb, sp = _table(m, tb).device(ctx.device, list(lr.FIELDS))
    cp = m._cparams(good)
    assert paint(m.handle, span.start, span.end, null0, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # outputs[0] NULL
    assert paint_spans(m.handle, span.start, span.end, null0, None, C.byref(cp), sp, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # end < start
    assert paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # no images
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), None, 0) == abi.ZH_ERR_INVALID          # no params
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, 0) == abi.ZH_ERR_INVALID  # no table
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.HARD_SQUARE_SPAN_NOTE_ON] = abi.ScriptSpanParam(sp[abi.HARD_SQUARE_SPAN_FREQ].f, None)   # `f` on a u-only field
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    empty = abi.ScriptSpanTable(0, 0, ctb.count, ctb.start, ctb.end, ctb.note_id_changed)   # max_spans == 0
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(empty), 0) == abi.ZH_ERR_INVALID
    ctx.sync()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and torch.equal(sync.view(torch.int32), sbefore.view(torch.int32))
    assert m.state().tobytes() == state                                                   # nothing painted
    m.close()
