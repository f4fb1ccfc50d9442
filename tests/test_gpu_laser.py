"""GPU: the sound-effect voice -- zh_sfx_kit, zh_laser_paint (k_laser) and zh_laser_paint_spans (k_laser_spans) -- against
tests/laser_reference.py: LaserPlayer.paint as the literal sequence of oracle calls, per voice and per sub-span.  Everything on
bits: the uint32 views of the images and of the five modules' state."""
import ctypes as C

import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import laser_cases as lc
from tests import laser_reference as lr
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kits(ctx):
    from zang_amd.sfx import SfxKit
    k = SfxKit(ctx, lc.kit_effects())
    yield lr.Kit(lc.kit_effects()), k
    k.close()


def _table(m, tb, names=lr.FIELDS):
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], lc.span_values(tb, names) if names else None)


def _check(m, out, ref, voices, what):
    util.assert_bitexact(util.from_image(out), ref, what)
    util.assert_bitexact(lr.struct_state(m.state()), lr.state_words(voices), what + " state")


@pytest.mark.parametrize("V", [1, 64, 65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_equals_the_reference_per_sub_span(ctx, oracle, kits, V, zero_first):
    """Two consecutive buffers with carried state, all five fields from span arrays: empty sub-spans, one out of order, effects
    that change without note_id_changed, the kit's count as an index, a voice with no sub-span; rows outside [3, 250) keep their
    bits and -0.0 planted in the base survives exactly where the reference leaves it."""
    from zang_amd import modules as mod, zang
    rk, gk = kits
    m = mod.Laser(V, ctx)
    voices = [lr.Voice(oracle) for _ in range(V)]
    for b in range(2):
        tb = lc.tables(V, 1000 * V + b, second=b == 1)
        base = lc.base_image(V, 77 + V + b)
        ref = lr.paint_spans(oracle, rk, voices, tb, base.copy(), lc.SPAN, lc.SR, zero_first)
        out = util.to_image(base)
        m.paint_spans(zang.Span(*lc.SPAN), [out], None, m.Params(gk, lc.SR, 9.0, 9.0, 9.0, 9.0, 99), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_laser_spans"], ctx.last_form()
        _check(m, out, ref, voices, f"V={V} buffer {b}")
        if V > 1:
            assert not lc.same_bits(ref, base)
    m.close()


@pytest.mark.parametrize("mode", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, kits, mode):
    """broadcast: no span arrays at all (span_params NULL), one value of every field for every voice.  per_voice: all five from
    per-voice device arrays.  mixed: freq_mul and effect per sub-span, the other three per voice."""
    import torch
    from zang_amd import modules as mod, zang
    rk, gk = kits
    V = 65
    tb = lc.tables(V, 4242)
    m = mod.Laser(V, ctx)
    voices = [lr.Voice(oracle) for _ in range(V)]
    rng = np.random.default_rng(5)
    if mode == "broadcast":
        dflt = {"freq_mul": np.float32(1.1), "carrier_mul": np.float32(2.0), "modulator_mul": np.float32(0.5), "modulator_rad": np.float32(0.625), "effect": 1}
        params = m.Params(gk, lc.SR, 1.1, 2.0, 0.5, 0.625, 1)
        names = ()
    else:
        dflt = {n: rng.uniform(0.25, 4.0, V).astype(np.float32) for n in lr.FIELDS[:4]}
        dflt["effect"] = (np.arange(V) * 5 % 6).astype(np.uint32)
        params = m.Params(gk, lc.SR, *(util.dev(dflt[n]) for n in lr.FIELDS[:4]), torch.from_numpy(dflt["effect"].astype(np.int32)).cuda())
        names = () if mode == "per_voice" else ("freq_mul", "effect")
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base = lc.base_image(V, 3)
    ref = lr.paint_spans(oracle, rk, voices, lean, base.copy(), lc.SPAN, lc.SR, False, dflt=dflt)
    out = util.to_image(base)
    m.paint_spans(zang.Span(*lc.SPAN), [out], None, params, _table(m, tb, names))
    ctx.sync()
    _check(m, out, ref, voices, mode)
    assert not lc.same_bits(ref, base)
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_uniform_paint_equals_the_span_form_with_one_full_sub_span(ctx, oracle, kits, V, monkeypatch):
    """zh_laser_paint: V LaserPlayers, each with its own effect, scalars and note_id_changed, painting the span twice (ADD, then
    ZERO_FIRST) with carried state == the reference == zh_laser_paint_spans over one full sub-span per voice == the same paint
    through the walk (dispatch row laser_uniform_walk)"""
    import torch
    from zang_amd import modules as mod, zang
    rk, gk = kits
    S, E = lc.SPAN
    ms = [mod.Laser(V, ctx) for _ in range(3)]
    voices = [lr.Voice(oracle) for _ in range(V)]
    for b in range(2):
        one = lc.tables(V, 77 * V + b)
        tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
              "nic": one["nic"][:1], **{n: one[n][b:b + 1] for n in lr.FIELDS}}
        base = lc.base_image(V, 31 + V + b)
        ref = lr.paint_spans(oracle, rk, voices, tb, base.copy(), lc.SPAN, lc.SR, b == 1)
        params = ms[0].Params(gk, lc.SR, *(util.dev(tb[n][0]) for n in lr.FIELDS[:4]), torch.from_numpy(tb["effect"][0].astype(np.int32)).cuda())
        outs = [util.to_image(base) for _ in range(3)]
        ms[0].paint(zang.Span(S, E), [outs[0]], [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_laser"], ctx.last_form()
        ms[1].paint_spans(zang.Span(S, E), [outs[1]], None, ms[1].Params(gk, lc.SR), _table(ms[1], tb), zero_first=b == 1)
        util.set_form(monkeypatch, laser_uniform_walk=1)
        ms[2].paint(zang.Span(S, E), [outs[2]], [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_laser_spans"], ctx.last_form()
        util.del_form(monkeypatch, "laser_uniform_walk")
        for i, what in enumerate(("uniform", "one sub-span", "uniform through the walk")):
            _check(ms[i], outs[i], ref, voices, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


def test_the_references_triple_over_ten_buffers(ctx, oracle):
    """the 0.2 s curves of example_laser.zig:22-38 over ten buffers of 1,024 frames at 65 voices, each with its own scalars; the
    impulse is buffer 0's note_id_changed"""
    from zang_amd import modules as mod, sfx, zang
    V, F = 65, 1024
    rk, gk = lr.Kit(lc.default_kit_effects()), sfx.SfxKit(ctx, lc.default_kit_effects())
    rng = np.random.default_rng(11)
    vals = {"freq_mul": rng.uniform(0.85, 1.15, V).astype(np.float32), "carrier_mul": rng.choice([2.0, 4.0, 0.5, 1.0], V).astype(np.float32),
            "modulator_mul": rng.choice([0.5, 0.125, 9.0], V).astype(np.float32), "modulator_rad": rng.uniform(0.375, 1.0, V).astype(np.float32)}
    m = mod.Laser(V, ctx)
    params = m.Params(gk, lc.SR, *(util.dev(vals[n]) for n in lr.FIELDS[:4]), 0)
    voices = [lr.Voice(oracle) for _ in range(V)]
    temps = [np.zeros(F, np.float32) for _ in range(3)]
    loud = 0.0
    for b in range(10):
        ref = np.zeros((V, F), np.float32)
        for v in range(V):
            lr.laser_paint(oracle, voices[v], rk, 0, F, ref[v], temps, b == 0, lc.SR, *(vals[n][v] for n in lr.FIELDS[:4]), 0)
        out = ctx.image(F, V, fill=0.0)
        m.paint(zang.Span(0, F), [out], [], b == 0, params)
        ctx.sync()
        _check(m, out, ref, voices, f"buffer {b}")
        loud = max(loud, float(np.abs(ref).max()))
        if b == 9:
            assert not (ref.view(np.uint32)[:, 384:] & 0x7FFFFFFF).any()       # 9,600 frames = 0.2 s: silence from there on
    assert loud > 0.5
    m.close(); gk.close()


HOSTILE = [np.nan, np.inf, -np.inf, 1e30]


def _hostile_run(ctx, oracle, kits, V, vals, effect, sample_rate, what):
    """two uniform paints with carried state (note_id_changed, then clear), per-voice scalars; NaN payloads excepted exactly as
    tests/test_gpu_hostile_params.py treats them (hostile_cases.same_f32)"""
    import torch
    from zang_amd import modules as mod, zang
    rk, gk = kits
    S, E = lc.SPAN
    m = mod.Laser(V, ctx)
    voices = [lr.Voice(oracle) for _ in range(V)]
    temps = [np.zeros(lc.ROWS, np.float32) for _ in range(3)]
    params = m.Params(gk, sample_rate, *(util.dev(vals[n]) for n in lr.FIELDS[:4]), torch.from_numpy(effect.astype(np.int32)).cuda())
    painted = 0
    for b in range(2):
        base = lc.base_image(V, 900 + b)
        ref = base.copy()
        for v in range(V):
            lr.laser_paint(oracle, voices[v], rk, S, E, ref[v], temps, b == 0, sample_rate, *(vals[n][v] for n in lr.FIELDS[:4]), int(effect[v]))
        out = util.to_image(base)
        m.paint(zang.Span(S, E), [out], [], b == 0, params)
        ctx.sync()
        got = util.from_image(out)
        assert hc.same_f32(got, ref), (what, b, hc.first_difference(got, ref))
        gs, rs = lr.struct_state(m.state()), lr.state_words(voices)
        for j, (_, field) in enumerate(lr.Voice.STATE):
            if field == "t":
                assert hc.same_f32(gs[:, j].view(np.float32), rs[:, j].view(np.float32)), (what, b, j, gs[:, j], rs[:, j])
            else:
                assert np.array_equal(gs[:, j], rs[:, j]), (what, b, j, gs[:, j], rs[:, j])
        painted += int((~lc_same(ref, base)).sum())
    assert painted > 0
    m.close()


def lc_same(a, b):
    return a.view(np.uint32) == b.view(np.uint32)


def test_hostile_multipliers_equal_the_reference(ctx, oracle, kits):
    """NaN, +/-inf and 1e30 in each of the four multipliers, one voice each, on effects 0, 1 and 4; two ordinary voices beside them"""
    V = len(HOSTILE) * 4 + 2
    vals = {"freq_mul": np.full(V, 1.0, np.float32), "carrier_mul": np.full(V, 2.0, np.float32), "modulator_mul": np.full(V, 0.5, np.float32),
            "modulator_rad": np.full(V, 0.5, np.float32)}
    for f, name in enumerate(lr.FIELDS[:4]):
        vals[name][f * len(HOSTILE):(f + 1) * len(HOSTILE)] = HOSTILE
    effect = np.array([0, 1, 4])[np.arange(V) % 3].astype(np.uint32)
    _hostile_run(ctx, oracle, kits, V, vals, effect, lc.SR, "multipliers")


@pytest.mark.parametrize("sample_rate", [0.0, -48000.0, float("nan")], ids=["zero", "negative", "nan"])
def test_hostile_sample_rates_equal_the_reference(ctx, oracle, kits, sample_rate):
    V = 5
    vals = {"freq_mul": np.full(V, 1.0, np.float32), "carrier_mul": np.full(V, 2.0, np.float32), "modulator_mul": np.full(V, 0.5, np.float32),
            "modulator_rad": np.full(V, 0.5, np.float32)}
    _hostile_run(ctx, oracle, kits, V, vals, np.arange(V).astype(np.uint32), sample_rate, f"sample_rate {sample_rate}")


def test_state_round_trip_and_a_carried_index_past_the_kit(ctx, oracle, kits):
    """get_state after set_state gives the words back; a current_song_note that only set_state can produce, past the kit's node
    array, is dropped instead of read (include/zang_hip.h), as the reference restates it"""
    from zang_amd import modules as mod, zang
    rk, gk = kits
    V = 3
    m = mod.Laser(V, ctx)
    st = m.state()
    rng = np.random.default_rng(2)
    for obj, field in lr.Voice.STATE:
        col = st[obj][field]
        col[:] = rng.uniform(0.0, 1.0, V).astype(np.float32) if field == "t" else rng.integers(0, 3, V).astype(col.dtype)
    st["volume_curve"]["current_song_note"][:] = [10 ** 6, 0, 1]
    st["volume_curve"]["next_song_note"][:] = [10 ** 6 + 1, 1, 2]
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    voices = [lr.Voice(oracle) for _ in range(V)]
    for v in range(V):
        for obj, field in lr.Voice.STATE:
            setattr(getattr(voices[v], obj), field, st[obj][field][v].item())
    S, E = lc.SPAN
    base = lc.base_image(V, 8)
    ref = base.copy()
    temps = [np.zeros(lc.ROWS, np.float32) for _ in range(3)]
    for v in range(V):
        lr.laser_paint(oracle, voices[v], rk, S, E, ref[v], temps, False, lc.SR, 1.0, 2.0, 0.5, 0.5, 0)
    out = util.to_image(base)
    m.paint(zang.Span(S, E), [out], [], False, m.Params(gk, lc.SR, 1.0, 2.0, 0.5, 0.5, 0))
    ctx.sync()
    _check(m, out, ref, voices, "carried index past the kit")
    m.close()


def test_paints_span_paints_and_a_graph_replay_mix(oracle):
    """a span paint, a captured span paint replayed twice and a uniform paint of ONE zh_laser == the same four paints made
    directly on another (image and state)"""
    import torch
    import zang_amd
    from zang_amd import modules as mod, zang
    from zang_amd.sfx import SfxKit
    V = 65
    tb = lc.tables(V, 5150)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        k2 = SfxKit(c2, lc.kit_effects())
        me, mg = mod.Laser(V, c2), mod.Laser(V, c2)
        base = lc.base_image(V, 8)
        out_e, out_g = util.to_image(base), util.to_image(base)
        tab_e, tab_g = _table(me, tb), _table(mg, tb)
        tab_g.device(c2.device, list(lr.FIELDS))      # uploaded before the capture records
        span = zang.Span(*lc.SPAN)
        spans = lambda m, out, tab: m.paint_spans(span, [out], None, m.Params(k2, lc.SR), tab)
        plain = lambda m, out: m.paint(span, [out], [], False, m.Params(k2, lc.SR, 1.0, 2.0, 0.5, 0.5, 1))
        for _ in range(3):
            spans(me, out_e, tab_e)
        plain(me, out_e)
        c2.sync()
        spans(mg, out_g, tab_g)
        g = c2.capture(lambda: spans(mg, out_g, tab_g))
        g.launch(); g.launch()
        plain(mg, out_g)
        c2.sync()
        assert torch.equal(out_e.view(torch.int32), out_g.view(torch.int32))
        assert me.state().tobytes() == mg.state().tobytes()
        assert not torch.equal(out_e, util.to_image(base))
        g.close(); me.close(); mg.close(); k2.close()
        c2.close()


def test_stage_by_stage_through_the_kits_device_pointers(ctx, kits):
    """zh_sfx_kit_effect hands out device pointers that zh_curve_module_paint takes: the volume curve of effect 0 painted by a
    Curve module == the node list painted from a tensor of the same nodes"""
    import torch
    from zang_amd import abi, modules as mod, zang
    _, gk = kits
    e = gk.effect(0)
    nodes, fn = lc.kit_effects()[0][2]
    assert (e.volume.count, e.volume.function) == (len(nodes), fn) and e.volume.nodes and e.modulator.nodes
    V = 4
    a, b = mod.Curve(V, ctx), mod.Curve(V, ctx)
    out_a, out_b = ctx.image(lc.ROWS, V, fill=0.0), ctx.image(lc.ROWS, V, fill=0.0)
    cp = abi.CurveModuleParams(lc.SR, fn, e.volume.nodes, e.volume.count)
    a._paint(zang.Span(*lc.SPAN), [out_a], [], True, cp, False)
    t = torch.tensor([[v, tt] for tt, v in nodes], dtype=torch.float32).cuda()
    b.paint(zang.Span(*lc.SPAN), [out_b], [], True, b.Params(lc.SR, fn, t))
    ctx.sync()
    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)) and float(out_a.abs().max()) > 0.5
    n = C.c_uint32()
    assert ctx.lib.zh_sfx_kit_count(gk.handle, C.byref(n)) == 0 and n.value == 5 == gk.count
    a.close(); b.close()


def test_refusals(ctx, kits):
    import torch
    import zang_amd
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf
    from zang_amd.sfx import SfxKit
    _, gk = kits
    V = 8
    tb = lc.tables(V, 1)
    m = mod.Laser(V, ctx)
    out = ctx.image(lc.ROWS, V, fill=0.25)
    before = out.clone()
    state = m.state().tobytes()
    span = zang.Span(*lc.SPAN)
    good = m.Params(gk, lc.SR)
    assert m._paint_spans(span, [out], None, good, _table(m, tb), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_spans(span, [out[:50]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID      # too few rows
    assert m._paint_spans(span, [out[:, :V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID  # too few voices
    with pytest.raises(abi.ZangHipError):
        m.paint(span, [out[:50]], [], False, good)
    outs = (abi.Buf * 1)(as_buf(out))
    ctb, sp = _table(m, tb).device(ctx.device, list(lr.FIELDS))
    cp = abi.LaserParams()                                              # a NULL kit
    assert ctx.lib.zh_laser_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_laser_paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID
    cp = m._cparams(good)
    assert ctx.lib.zh_laser_paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert ctx.lib.zh_laser_paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # end < start
    assert ctx.lib.zh_laser_paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # no image
    assert ctx.lib.zh_laser_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, 0) == abi.ZH_ERR_INVALID  # no table
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.LASER_SPAN_EFFECT] = abi.ScriptSpanParam(sp[abi.LASER_SPAN_FREQ_MUL].f, None)   # `f` on the u-only field
    assert ctx.lib.zh_laser_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    empty = abi.ScriptSpanTable(0, 0, ctb.count, ctb.start, ctb.end, ctb.note_id_changed)   # max_spans == 0
    assert ctx.lib.zh_laser_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(empty), 0) == abi.ZH_ERR_INVALID
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        other = SfxKit(c2, lc.kit_effects())                             # a kit of another context
        assert m._paint_spans(span, [out], None, m.Params(other, lc.SR), _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID
        other.close(); c2.close()
    nodes = (abi.CurveNode * 2)()
    h = C.c_void_p()
    ok = abi.SfxCurve(C.addressof(nodes), 2, 1)
    for e, n in ((abi.SfxEffect(ok, ok, ok), 0),                                                       # no effects
                 (abi.SfxEffect(ok, abi.SfxCurve(None, 2, 1), ok), 1),                                 # nodes promised, none given
                 (abi.SfxEffect(ok, ok, abi.SfxCurve(C.addressof(nodes), 2, 2)), 1)):                  # a function outside the enum
        assert ctx.lib.zh_sfx_kit_create(ctx.handle, C.byref(e), n, C.byref(h)) == abi.ZH_ERR_INVALID and not h.value
    ctx.sync()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and m.state().tobytes() == state   # nothing painted
    m.close()
