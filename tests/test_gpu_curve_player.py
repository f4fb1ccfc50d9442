"""GPU: the curve voice -- zh_curve_player_paint and zh_curve_player_paint_spans, one kernel (k_curve_player_spans) -- against
tests/curve_player_reference.py: CurvePlayer.paint as the literal sequence of oracle calls, per voice and per sub-span.
Everything on bits: the uint32 views of both images and of the four modules' ten state words."""
import ctypes as C

import numpy as np
import pytest

from tests import curve_player_cases as cc
from tests import curve_player_reference as cr
from tests import hostile_cases as hc
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kits(ctx):
    from zang_amd.sfx import SfxKit
    k = SfxKit(ctx, cc.kit_effects())
    yield cr.Kit(cc.kit_effects()), k
    k.close()


def _table(m, tb, names=cr.FIELDS):
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], cc.span_values(tb, names) if names else None)


def _check(m, outs, refs, voices, what):
    for i, (out, ref) in enumerate(zip(outs, refs)):
        util.assert_bitexact(util.from_image(out), ref, f"{what} outputs[{i}]")
    util.assert_bitexact(cr.struct_state(m.state()), cr.state_words(voices), what + " state")


@pytest.mark.parametrize("V", [1, 64, 65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
@pytest.mark.parametrize("sync", [True, False], ids=["two_outputs", "one_output"])
def test_span_paint_equals_the_reference_per_sub_span(ctx, oracle, kits, V, zero_first, sync):
    """Two consecutive buffers with carried state, both fields from span arrays: empty sub-spans, one out of order, effects that
    change without note_id_changed, the kit's count as an index, a voice with no sub-span; rows outside [3, 250) keep their bits
    and -0.0 planted in either base survives exactly where the reference leaves it.  Without outputs[1] the image that would
    have been it is untouched."""
    from zang_amd import modules as mod, zang
    rk, gk = kits
    S, E = cc.SPAN
    m = mod.CurveVoice(V, ctx)
    voices = [cr.Voice(oracle) for _ in range(V)]
    for b in range(2):
        tb = cc.tables(V, 1000 * V + b, second=b == 1)
        base0, base1 = cc.base_image(V, 77 + V + b), cc.base_image(V, 177 + V + b)
        ref0, ref1 = cr.paint_spans(oracle, rk, voices, tb, base0.copy(), base1.copy() if sync else None, cc.SPAN, cc.SR, zero_first)
        out0, out1 = util.to_image(base0), util.to_image(base1)
        m.paint_spans(zang.Span(S, E), [out0, out1] if sync else [out0], None, m.Params(gk, cc.SR, 9.0, 99), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_curve_player_spans"], ctx.last_form()
        _check(m, [out0, out1], [ref0, ref1 if sync else base1], voices, f"V={V} buffer {b}")
        for ref, base in ((ref0, base0), (ref1 if sync else base1, base1)):
            assert cc.same_bits(ref[:, :S], base[:, :S]) and cc.same_bits(ref[:, E:], base[:, E:])
        if V > 1:
            assert not cc.same_bits(ref0, base0) and (not sync or not cc.same_bits(ref1, base1))
    m.close()


@pytest.mark.parametrize("mode", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, kits, mode):
    """broadcast: no span arrays at all (span_params NULL), one value of both fields for every voice.  per_voice: both from
    per-voice device arrays.  mixed: the effect per sub-span, rel_freq per voice."""
    import torch
    from zang_amd import modules as mod, zang
    rk, gk = kits
    V = 65
    tb = cc.tables(V, 4242)
    m = mod.CurveVoice(V, ctx)
    voices = [cr.Voice(oracle) for _ in range(V)]
    rng = np.random.default_rng(5)
    if mode == "broadcast":
        dflt = {"rel_freq": np.float32(1.1), "effect": 1}
        params = m.Params(gk, cc.SR, 1.1, 1)
        names = ()
    else:
        dflt = {"rel_freq": rng.uniform(0.25, 4.0, V).astype(np.float32), "effect": (np.arange(V) * 5 % 6).astype(np.uint32)}
        params = m.Params(gk, cc.SR, util.dev(dflt["rel_freq"]), torch.from_numpy(dflt["effect"].astype(np.int32)).cuda())
        names = () if mode == "per_voice" else ("effect",)
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base0, base1 = cc.base_image(V, 3), cc.base_image(V, 4)
    ref0, ref1 = cr.paint_spans(oracle, rk, voices, lean, base0.copy(), base1.copy(), cc.SPAN, cc.SR, False, dflt=dflt)
    out0, out1 = util.to_image(base0), util.to_image(base1)
    m.paint_spans(zang.Span(*cc.SPAN), [out0, out1], None, params, _table(m, tb, names))
    ctx.sync()
    _check(m, [out0, out1], [ref0, ref1], voices, mode)
    assert not cc.same_bits(ref0, base0) and not cc.same_bits(ref1, base1)
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_plain_paint_equals_the_span_form_with_one_full_sub_span(ctx, oracle, kits, V):
    """zh_curve_player_paint: V CurvePlayers, each with its own effect, rel_freq and note_id_changed, painting the span twice (ADD,
    then ZERO_FIRST) with carried state == the reference == zh_curve_player_paint_spans over one full sub-span per voice; the same
    kernel both ways"""
    import torch
    from zang_amd import modules as mod, zang
    rk, gk = kits
    S, E = cc.SPAN
    ms = [mod.CurveVoice(V, ctx) for _ in range(2)]
    voices = [cr.Voice(oracle) for _ in range(V)]
    for b in range(2):
        one = cc.tables(V, 77 * V + b)
        tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
              "nic": one["nic"][:1], **{n: one[n][b:b + 1] for n in cr.FIELDS}}
        base0, base1 = cc.base_image(V, 31 + V + b), cc.base_image(V, 131 + V + b)
        ref0, ref1 = cr.paint_spans(oracle, rk, voices, tb, base0.copy(), base1.copy(), cc.SPAN, cc.SR, b == 1)
        params = ms[0].Params(gk, cc.SR, util.dev(tb["rel_freq"][0]), torch.from_numpy(tb["effect"][0].astype(np.int32)).cuda())
        outs = [(util.to_image(base0), util.to_image(base1)) for _ in range(2)]
        ms[0].paint(zang.Span(S, E), list(outs[0]), [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_curve_player_spans"], ctx.last_form()
        ms[1].paint_spans(zang.Span(S, E), list(outs[1]), None, ms[1].Params(gk, cc.SR), _table(ms[1], tb), zero_first=b == 1)
        ctx.sync()
        for i, what in enumerate(("plain", "one sub-span")):
            _check(ms[i], outs[i], [ref0, ref1], voices, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


def test_out_of_range_effect_under_note_id_changed_touches_nothing(ctx, kits):
    """effect == the kit's count and beyond, note_id_changed set, on voices that carry a sound: both outputs and the ten words keep
    their bits (an ADD paint; ZERO_FIRST writes its zeros and leaves the state)"""
    import torch
    from zang_amd import modules as mod, zang
    _, gk = kits
    V = 65
    S, E = cc.SPAN
    m = mod.CurveVoice(V, ctx)
    out0, out1 = ctx.image(cc.ROWS, V, fill=0.0), ctx.image(cc.ROWS, V, fill=0.0)
    m.paint(zang.Span(S, 100), [out0, out1], [], True, m.Params(gk, cc.SR, 1.0, 0))
    ctx.sync()
    state = m.state().tobytes()
    assert float(out0.abs().max()) > 0.5 and any(state)
    before = out0.clone(), out1.clone()
    bad = torch.from_numpy((5 + np.arange(V) * 1000003 % (2 ** 31 - 5)).astype(np.int32)).cuda()
    m.paint(zang.Span(S, E), [out0, out1], [], True, m.Params(gk, cc.SR, 2.0, bad))
    ctx.sync()
    assert torch.equal(out0.view(torch.int32), before[0].view(torch.int32)) and torch.equal(out1.view(torch.int32), before[1].view(torch.int32))
    assert m.state().tobytes() == state
    m.paint(zang.Span(S, E), [out0, out1], [], True, m.Params(gk, cc.SR, 2.0, 5), zero_first=True)
    ctx.sync()
    for out, was in zip((out0, out1), before):
        assert not out[S:E].view(torch.int32).any() and torch.equal(out[:S].view(torch.int32), was[:S].view(torch.int32))
    assert m.state().tobytes() == state
    m.close()


def test_state_round_trip_and_a_carried_index_past_the_kit(ctx, oracle, kits):
    """get_state after set_state gives the words back; a current_song_note that only set_state can produce, past the kit's node
    array, is dropped instead of read (include/zang_hip.h), as the reference restates it"""
    from zang_amd import modules as mod, zang
    rk, gk = kits
    V = 3
    m = mod.CurveVoice(V, ctx)
    st = m.state()
    rng = np.random.default_rng(2)
    for obj, field in cr.Voice.STATE:
        col = st[obj][field]
        col[:] = rng.uniform(0.0, 1.0, V).astype(np.float32) if field == "t" else rng.integers(0, 3, V).astype(col.dtype)
    st["carrier_curve"]["current_song_note"][:] = [10 ** 6, 0, 1]
    st["carrier_curve"]["next_song_note"][:] = [10 ** 6 + 1, 1, 2]
    st["modulator_curve"]["current_song_note"][:] = [1, 2 ** 31, 0]
    st["modulator_curve"]["next_song_note"][:] = [2, 2 ** 31 + 1, 1]
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    voices = [cr.Voice(oracle) for _ in range(V)]
    for v in range(V):
        for obj, field in cr.Voice.STATE:
            setattr(getattr(voices[v], obj), field, st[obj][field][v].item())
    S, E = cc.SPAN
    base0, base1 = cc.base_image(V, 8), cc.base_image(V, 9)
    ref0, ref1 = base0.copy(), base1.copy()
    temps = [np.zeros(cc.ROWS, np.float32) for _ in range(2)]
    for v in range(V):
        cr.curve_player_paint(oracle, voices[v], rk, S, E, ref0[v], ref1[v], temps, False, cc.SR, 1.25, 0)
    out0, out1 = util.to_image(base0), util.to_image(base1)
    m.paint(zang.Span(S, E), [out0, out1], [], False, m.Params(gk, cc.SR, 1.25, 0))
    ctx.sync()
    _check(m, [out0, out1], [ref0, ref1], voices, "carried index past the kit")
    m.close()


HOSTILE_REL_FREQ = [np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-40, 1e30]


def test_hostile_rel_freq_equals_the_reference(ctx, oracle, kits):
    """NaN, +/-inf, -0.0, denormals and 1e30 as rel_freq, one voice each per effect among ordinary voices, V = 65, one buffer of
    the shared tables; on bits, any NaN equal to any NaN (tests/hostile_cases.same_f32).  -0.0 makes every f_c a -0.0: the
    frequency image keeps a planted -0.0 exactly there."""
    from zang_amd import modules as mod, zang
    rk, gk = kits
    V = 65
    tb = cc.tables(V, 31337)
    rel = tb["rel_freq"]
    for j, x in enumerate(HOSTILE_REL_FREQ * 5):
        rel[:, 5 + j] = np.float32(x)                              # voices 5..39: effect (v + k) % 6 walks every effect past each value
    m = mod.CurveVoice(V, ctx)
    voices = [cr.Voice(oracle) for _ in range(V)]
    base0, base1 = cc.base_image(V, 900), cc.base_image(V, 901)
    with np.errstate(all="ignore"):
        ref0, ref1 = cr.paint_spans(oracle, rk, voices, tb, base0.copy(), base1.copy(), cc.SPAN, cc.SR, False)
    out0, out1 = util.to_image(base0), util.to_image(base1)
    m.paint_spans(zang.Span(*cc.SPAN), [out0, out1], None, m.Params(gk, cc.SR), _table(m, tb))
    ctx.sync()
    for got, ref, what in ((util.from_image(out0), ref0, "outputs[0]"), (util.from_image(out1), ref1, "outputs[1]")):
        assert hc.same_f32(got, ref), (what, hc.first_difference(got, ref))
    gs, rs = cr.struct_state(m.state()), cr.state_words(voices)
    for j, (_, field) in enumerate(cr.Voice.STATE):
        if field == "t":
            assert hc.same_f32(gs[:, j].view(np.float32), rs[:, j].view(np.float32)), (j, gs[:, j], rs[:, j])
        else:
            assert np.array_equal(gs[:, j], rs[:, j]), (j, gs[:, j], rs[:, j])
    assert np.isnan(ref0).any() and np.isnan(ref1).any() and np.isinf(ref1).any()
    walk = [w for w in cc.walked(tb, V) if rel[w[1], w[0]].view(np.uint32) == 0x80000000 and w[5] < 5 and w[3] > w[2]]
    assert walk and any((ref1[v, s:e].view(np.uint32) == 0x80000000).any() for v, _, s, e, _, _ in walk)
    m.close()


def test_paints_span_paints_and_a_graph_replay_mix(oracle):
    """one captured graph of two span paints replayed twice == four direct span paints, with a plain paint after either (images
    and state)"""
    import torch
    import zang_amd
    from zang_amd import modules as mod, zang
    from zang_amd.sfx import SfxKit
    V = 65
    tb = cc.tables(V, 5150)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        k2 = SfxKit(c2, cc.kit_effects())
        me, mg = mod.CurveVoice(V, c2), mod.CurveVoice(V, c2)
        base0, base1 = cc.base_image(V, 8), cc.base_image(V, 9)
        outs_e, outs_g = [util.to_image(base0), util.to_image(base1)], [util.to_image(base0), util.to_image(base1)]
        tab_e, tab_g = _table(me, tb), _table(mg, tb)
        tab_g.device(c2.device, list(cr.FIELDS))      # uploaded before the capture records
        span = zang.Span(*cc.SPAN)
        spans = lambda m, outs, tab: m.paint_spans(span, outs, None, m.Params(k2, cc.SR), tab)
        plain = lambda m, outs: m.paint(span, outs, [], False, m.Params(k2, cc.SR, 1.25, 1))
        for _ in range(4):
            spans(me, outs_e, tab_e)
        plain(me, outs_e)
        c2.sync()
        g = c2.capture(lambda: (spans(mg, outs_g, tab_g), spans(mg, outs_g, tab_g)))
        g.launch(); g.launch()
        plain(mg, outs_g)
        c2.sync()
        for a, b, base in zip(outs_e, outs_g, (base0, base1)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, util.to_image(base))
        assert me.state().tobytes() == mg.state().tobytes()
        g.close(); me.close(); mg.close(); k2.close()
        c2.close()


def test_refusals(ctx, kits):
    import torch
    import zang_amd
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf
    from zang_amd.sfx import SfxKit
    _, gk = kits
    V = 8
    tb = cc.tables(V, 1)
    m = mod.CurveVoice(V, ctx)
    out0, out1 = ctx.image(cc.ROWS, V, fill=0.25), ctx.image(cc.ROWS, V, fill=0.5)
    before = out0.clone(), out1.clone()
    state = m.state().tobytes()
    span = zang.Span(*cc.SPAN)
    good = m.Params(gk, cc.SR)
    table = lambda: _table(m, tb)
    assert m._paint_spans(span, [out0, out1], None, good, table(), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_spans(span, [out0[:50], out1], None, good, table(), abi.PAINT_ADD) == abi.ZH_ERR_INVALID        # outputs[0]: too few rows
    assert m._paint_spans(span, [out0, out1[:50]], None, good, table(), abi.PAINT_ADD) == abi.ZH_ERR_INVALID        # a small outputs[1]
    assert m._paint_spans(span, [out0, out1[:, :V - 1]], None, good, table(), abi.PAINT_ADD) == abi.ZH_ERR_INVALID  # too few voices
    wide, marker = ctx.image(cc.ROWS, 2 * V, fill=0.5), ctx.last_form()    # outputs[1] shares a float with outputs[0]: refused, no launch
    assert m._paint_spans(span, [out0, out0], None, good, table(), abi.PAINT_ADD) == abi.ZH_ERR_INVALID                  # the same image
    assert m._paint_spans(span, [wide[:, :V], wide[:, V - 1:2 * V - 1]], None, good, table(), abi.PAINT_ADD) == abi.ZH_ERR_INVALID   # one column in common
    assert ctx.last_form() == marker
    with pytest.raises(abi.ZangHipError):
        m.paint(span, [out0, out1[:50]], [], False, good)
    outs = (abi.Buf * 2)(as_buf(out0), as_buf(out1))
    ctb, sp = table().device(ctx.device, list(cr.FIELDS))
    cp = abi.CurvePlayerParams()                                        # a NULL kit
    assert ctx.lib.zh_curve_player_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_curve_player_paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID
    cp = m._cparams(good)
    paint = ctx.lib.zh_curve_player_paint
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID      # end < start
    assert paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID      # no images
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), None, 0) == abi.ZH_ERR_INVALID             # no params
    assert ctx.lib.zh_curve_player_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, 0) == abi.ZH_ERR_INVALID  # no table
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.CURVE_PLAYER_SPAN_EFFECT] = abi.ScriptSpanParam(sp[abi.CURVE_PLAYER_SPAN_REL_FREQ].f, None)   # `f` on the u-only field
    assert ctx.lib.zh_curve_player_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    empty = abi.ScriptSpanTable(0, 0, ctb.count, ctb.start, ctb.end, ctb.note_id_changed)   # max_spans == 0
    assert ctx.lib.zh_curve_player_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(empty), 0) == abi.ZH_ERR_INVALID
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        other = SfxKit(c2, cc.kit_effects())                             # a kit of another context
        assert m._paint_spans(span, [out0, out1], None, m.Params(other, cc.SR), table(), abi.PAINT_ADD) == abi.ZH_ERR_INVALID
        other.close(); c2.close()
    ctx.sync()
    assert torch.equal(out0.view(torch.int32), before[0].view(torch.int32)) and torch.equal(out1.view(torch.int32), before[1].view(torch.int32))
    assert m.state().tobytes() == state                                  # nothing painted
    m.close()
