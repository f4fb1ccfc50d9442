"""GPU: the subsong example's inner voice -- zh_saw_env_paint[_spans] (k_saw_env_spans) -- against the composition the reference
performs, twice: through the existing entry points (zh_zero, zh_trisawosc_paint_spans, zh_zero, zh_envelope_paint_spans,
zh_multiply) and through the oracle's modules per voice and per sub-span (tests/subsong_reference.py inner_paint under
tests/lead_reference.py's Trigger loop).  Everything on bits: the uint32 views of the output image and the six state words after
every buffer; any NaN equals any NaN (by position).  Sub-spans of 1, 63 and 257 frames in every order, 1, 65 and 130 voices."""
import itertools

import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import lead_reference as lr
from tests import subsong_reference as sr
from tests import util

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 4000.0                                        # the oscillator paints 0 .. SR / 8 = 500 Hz
ROWS, SPAN = 340, (3, 337)
LENGTHS = (1, 63, 257)
VOICES = [1, 65, 130]
PATCH = (0.3, 0.004, 0.01, 0.02, 0.25)             # a triangle-ish colour and stages short enough to end inside 63 frames


def _paint(o, voice, s, e, outs, temps, nic, sample_rate, freq, note_on, patch):
    sr.inner_paint(o, voice, s, e, outs[0], temps, nic, sample_rate, freq, note_on, patch)


def tables(V, seed, freq_range=(40.0, 480.0)):
    """K = 3 sub-spans per voice, lengths 1, 63 and 257 in the voice's own order, adjacent or a frame or two apart, the first at
    3 .. 6; voice v % 7 == 6 has two only.  freq and note_on per sub-span; note_id_changed mostly follows a note-on"""
    rng = np.random.default_rng(seed)
    perms = list(itertools.permutations(LENGTHS))
    tb = {"count": np.zeros(V, np.uint32), "start": np.zeros((3, V), np.uint32), "end": np.zeros((3, V), np.uint32),
          "nic": np.zeros((3, V), np.uint8), "freq": rng.uniform(*freq_range, (3, V)).astype(f32),
          "note_on": (rng.random((3, V)) < 0.7).astype(np.uint32)}
    for v in range(V):
        pos = SPAN[0] + v % 4
        n = 2 if v % 7 == 6 else 3
        for k, length in enumerate(perms[v % 6][:n]):
            pos += (v + k) % 3 if k else 0
            tb["start"][k, v], tb["end"][k, v] = pos, pos + length
            pos += length
        assert pos <= SPAN[1]
        tb["count"][v] = n
    tb["nic"][:] = (tb["note_on"] != 0) & (rng.random((3, V)) < 0.8)
    return tb


def base_image(V, seed, minus_zero=False):
    img = np.random.default_rng(seed).uniform(-1.0, 1.0, (V, ROWS)).astype(f32)
    if minus_zero:
        img[:, ::5] = -0.0
    return img


def _values(tb, names=lr.FIELDS):
    return {n: ((tb[n], None) if n == "freq" else (None, tb[n])) for n in names}


def _table(m, tb, names=lr.FIELDS):
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], _values(tb, names) if names else None)


def _voices(oracle, V):
    return [sr.InnerVoice(oracle) for _ in range(V)]


def _words(m):
    st = m.state()
    u = lambda a: np.ascontiguousarray(a).view(np.uint32) if a.dtype == f32 else a.astype(np.uint32)
    cols = [st["osc"]["cnt"], st["osc"]["t"], st["env"]["state"], st["env"]["t"], st["env"]["last_value"], st["env"]["start"]]
    return np.stack([u(np.ascontiguousarray(c)) for c in cols], 1).tolist()


def _check(m, out, ref, vs, what):
    got = util.from_image(out)
    assert hc.same_f32(got, ref), (what, hc.first_difference(got, ref))
    assert _words(m) == [v.words() for v in vs], what + " state"


def _composition(ctx, mods, tb, out, zero_first, patch=sr.DEFAULT_PATCH):
    """InnerInstrument.paint as five calls of today's entry points over the whole span; temps zeroed, so frames outside the
    sub-spans get += 0 * 0"""
    from zang_amd import zang
    tri, env, t0, t1 = mods
    span = zang.Span(*SPAN)
    color, attack, decay, release, sustain = patch
    zang.zero(span, t0, ctx)
    tri.paint_spans(span, [t0], [], tri.Params(SR, zang.constant(0.0), color), _table(tri, tb, ("freq",)))
    zang.zero(span, t1, ctx)
    env.paint_spans(span, [t1], [], env.Params(SR, zang.PaintCurve.cubed(attack), zang.PaintCurve.cubed(decay), zang.PaintCurve.cubed(release),
                                                 sustain, False), _table(env, tb, ("note_on",)))
    if zero_first:
        zang.zero(span, out, ctx)
    zang.multiply(span, out, t0, t1, ctx)


@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_equals_the_composition_and_the_oracle(ctx, oracle, V, zero_first):
    """two consecutive buffers with carried state, both fields from span arrays; rows outside [3, 337) keep their bits"""
    from zang_amd import modules as mod, zang
    m = mod.SawEnv(V, ctx)
    mods = (mod.TriSawOsc(V, ctx), mod.Envelope(V, ctx), ctx.image(ROWS, V), ctx.image(ROWS, V))
    vs = _voices(oracle, V)
    for b in range(2):
        tb = tables(V, 1000 * V + b)
        base = base_image(V, 77 + V + b)
        ref = lr.paint_spans(oracle, _paint, vs, tb, base.copy(), None, SPAN, SR, zero_first, None)
        out, comp = util.to_image(base), util.to_image(base)
        m.paint_spans(zang.Span(*SPAN), [out], None, m.Params(SR), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_saw_env_spans"], ctx.last_form()
        _check(m, out, ref, vs, f"V={V} buffer {b}")
        _composition(ctx, mods, tb, comp, zero_first)
        ctx.sync()
        got, want = util.from_image(out), util.from_image(comp)
        assert hc.same_f32(got, want), (f"buffer {b}: fused != the five calls", hc.first_difference(got, want))
        assert np.array_equal(m.state()["osc"]["cnt"], mods[0].state()["cnt"]) and m.state()["env"].tobytes() == mods[1].state().tobytes()
        assert float(np.abs(ref[:, SPAN[0]:SPAN[1]]).max()) > 0.05 and not hc.same_f32(ref, base)
    for o in (m, mods[0], mods[1]):
        o.close()


def test_every_frame_of_a_sub_span_is_added_to(ctx, oracle):
    """-0.0 planted in the base, frequencies either side of SR / 8 and below 0, envelopes that are idle (a note-off from the
    start): where a module paints nothing the zeroed temp still goes through the multiply-add, so -0.0 becomes +0.0 inside a
    sub-span and stays outside"""
    from zang_amd import modules as mod, zang
    V = 65
    tb = tables(V, 606)
    rng = np.random.default_rng(9)
    tb["freq"][:] = rng.choice(np.array([490.0, 499.0, 500.0, 501.0, 510.0, -1.0, -220.0, 220.0, 4000.0], f32), tb["freq"].shape)
    tb["note_on"][:, 1] = 0                                            # voice 1 never had a note: the envelope stays idle
    tb["freq"][:, 1] = 600.0                                           # ... and its oscillator is out of range throughout
    m = mod.SawEnv(V, ctx)
    vs = _voices(oracle, V)
    base = base_image(V, 12, minus_zero=True)
    ref = lr.paint_spans(oracle, _paint, vs, tb, base.copy(), None, SPAN, SR, False, None)
    out = util.to_image(base)
    m.paint_spans(zang.Span(*SPAN), [out], None, m.Params(SR), _table(m, tb))
    ctx.sync()
    _check(m, out, ref, vs, "nothing painted")
    k = int(np.argmax(tb["end"][:, 1] - tb["start"][:, 1]))            # voice 1's sub-span of 257 frames
    s, e = int(tb["start"][k, 1]), int(tb["end"][k, 1])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    inside, outside = np.arange(s, e)[np.arange(s, e) % 5 == 0], np.arange(0, SPAN[0])[::5]
    assert len(inside) > 50 and (bits(ref[1, inside]) == 0).all() and (bits(ref[1, outside]) == 0x80000000).all() and vs[1].words()[0] == 0
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_plain_paint_equals_the_oracle_and_the_span_form(ctx, oracle, V):
    """zh_saw_env_paint: V voices with their own freq and note_on over spans of 1, 63 and 257 frames (ADD, ZERO_FIRST, ADD) with
    carried state and note_id_changed on, off, on == the oracle == the span form over one full sub-span per voice"""
    from zang_amd import modules as mod, zang
    ms = [mod.SawEnv(V, ctx) for _ in range(2)]
    vs = _voices(oracle, V)
    rng = np.random.default_rng(V)
    pos = SPAN[0]
    for b, length in enumerate(LENGTHS):
        S, E = pos, pos + length
        pos = E
        nic = b != 1
        tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
              "nic": np.full((1, V), nic, np.uint8), "freq": rng.uniform(40.0, 480.0, (1, V)).astype(f32),
              "note_on": (np.arange(V)[None, :] % 3 != b).astype(np.uint32)}
        base = base_image(V, 31 + V + b, minus_zero=True)
        ref = lr.paint_spans(oracle, _paint, vs, tb, base.copy(), None, (S, E), SR, b == 1, None)
        outs = [util.to_image(base) for _ in range(2)]
        params = ms[0].Params(SR, util.dev(tb["freq"][0]), util.dev(tb["note_on"][0].astype(np.uint8)))
        ms[0].paint(zang.Span(S, E), [outs[0]], [], nic, params, zero_first=b == 1)
        ms[1].paint_spans(zang.Span(S, E), [outs[1]], None, ms[1].Params(SR), _table(ms[1], tb), zero_first=b == 1)
        ctx.sync()
        for i, what in enumerate(("plain", "one sub-span")):
            _check(ms[i], outs[i], ref, vs, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


@pytest.mark.parametrize("how", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, how):
    from zang_amd import modules as mod, zang
    V = 65
    tb = tables(V, 4242)
    m = mod.SawEnv(V, ctx)
    vs = _voices(oracle, V)
    rng = np.random.default_rng(5)
    if how == "broadcast":
        dflt, params, names = {"freq": f32(330.0), "note_on": 1}, m.Params(SR, 330.0, True), ()
    else:
        dflt = {"freq": rng.uniform(40.0, 480.0, V).astype(f32), "note_on": (np.arange(V) % 3 != 0).astype(np.uint32)}
        params = m.Params(SR, util.dev(dflt["freq"]), util.dev(dflt["note_on"].astype(np.uint8)))
        names = () if how == "per_voice" else ("freq",)
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base = base_image(V, 3)
    ref = lr.paint_spans(oracle, _paint, vs, lean, base.copy(), None, SPAN, SR, False, None, dflt=dflt)
    out = util.to_image(base)
    m.paint_spans(zang.Span(*SPAN), [out], None, params, _table(m, tb, names))
    ctx.sync()
    _check(m, out, ref, vs, how)
    m.close()


def test_a_patch_of_the_callers_and_an_output_view_with_an_odd_stride(ctx, oracle):
    """another colour (the triangle arms), stages that end inside a sub-span, a sustain volume of its own -- against the oracle
    and against the five calls -- into columns 2 .. V + 2 of an image whose rows are 69 floats apart"""
    from zang_amd import modules as mod, zang
    V = 65
    m = mod.SawEnv(V, ctx)
    mods = (mod.TriSawOsc(V, ctx), mod.Envelope(V, ctx), ctx.image(ROWS, V), ctx.image(ROWS, V))
    vs = _voices(oracle, V)
    patch = m.Patch(*PATCH)
    for b in range(2):
        tb = tables(V, 900 + b)
        base = base_image(V, 55 + b)
        ref = lr.paint_spans(oracle, _paint, vs, tb, base.copy(), None, SPAN, SR, False, PATCH)
        wide = ctx.image(ROWS, V + 4, fill=0.125)
        view = wide[:, 2:V + 2]
        assert view.stride(0) == 69
        view.copy_(util.to_image(base))
        m.paint_spans(zang.Span(*SPAN), [view], None, m.Params(SR, patch=patch), _table(m, tb))
        ctx.sync()
        _check(m, view, ref, vs, f"patch, buffer {b}")
        rim = wide.cpu().numpy()
        assert (rim[:, :2] == 0.125).all() and (rim[:, V + 2:] == 0.125).all()
        comp = util.to_image(base)
        _composition(ctx, mods, tb, comp, False, PATCH)
        ctx.sync()
        assert hc.same_f32(util.from_image(comp), ref), f"buffer {b}: the five calls"
    for o in (m, mods[0], mods[1]):
        o.close()


def test_state_round_trip(ctx, oracle):
    from zang_amd import modules as mod, zang
    V = 3
    m = mod.SawEnv(V, ctx)
    st = m.state()
    assert st.tobytes() == bytes(st.nbytes)                            # create == init(): every word zero
    st["osc"]["cnt"][:] = (1, 0x80000000, 0xfffffff0)
    st["osc"]["t"][:] = (0.25, -3.5, 1e9)                              # never read, never changed by the constant-frequency path
    st["env"]["state"][:] = (1, 3, 4)                                  # attack, sustain, release
    st["env"]["t"][:] = (0.5, 0.0, 0.25)
    st["env"]["last_value"][:] = (0.75, 0.5, 0.4)
    st["env"]["start"][:] = (0.1, 0.5, 0.5)
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    vs = _voices(oracle, V)
    for v in range(V):
        vs[v].osc.cnt, vs[v].osc.t = int(st["osc"]["cnt"][v]), float(st["osc"]["t"][v])
        vs[v].env.state = int(st["env"]["state"][v])
        vs[v].env.painter.t, vs[v].env.painter.last_value, vs[v].env.painter.start = (float(st["env"][k][v]) for k in ("t", "last_value", "start"))
    on = np.array([1, 1, 0], np.uint32)
    tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), SPAN[0], np.uint32), "end": np.full((1, V), SPAN[1], np.uint32),
          "nic": np.zeros((1, V), np.uint8), "freq": np.full((1, V), 220.0, f32), "note_on": on[None, :]}
    base = base_image(V, 8)
    ref = lr.paint_spans(oracle, _paint, vs, tb, base.copy(), None, SPAN, SR, False, None)
    out = util.to_image(base)
    m.paint(zang.Span(*SPAN), [out], [], False, m.Params(SR, 220.0, util.dev(on.astype(np.uint8))))
    ctx.sync()
    _check(m, out, ref, vs, "from a set state")
    m.close()


def test_refusals(ctx):
    import ctypes as C
    import torch
    from zang_amd import abi, modules as mod, zang
    V = 8
    tb = tables(V, 1)
    m = mod.SawEnv(V, ctx)
    out = ctx.image(ROWS, V, fill=0.25)
    before, state = out.clone(), m.state().tobytes()
    span, good = zang.Span(*SPAN), m.Params(SR)
    assert m._paint_spans(span, [out], None, good, _table(m, tb), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_spans(span, [out[:50]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID        # too few rows
    assert m._paint_spans(span, [out[:, :V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID  # too few voices
    with pytest.raises(abi.ZangHipError):
        m.paint(span, [out[:50]], [], False, good)
    paint, paint_spans = ctx.lib.zh_saw_env_paint, ctx.lib.zh_saw_env_paint_spans
    outs, cp = m._outputs([out]), m._cparams(good)
    ctb, sp = _table(m, tb).device(ctx.device, list(lr.FIELDS))
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID     # end < start
    assert paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), None, 0) == abi.ZH_ERR_INVALID
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, 0) == abi.ZH_ERR_INVALID
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.SAW_ENV_SPAN_NOTE_ON] = abi.ScriptSpanParam(sp[abi.SAW_ENV_SPAN_FREQ].f, None)                         # `f` on a u-only field
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    patch = abi.SawEnvPatch()
    assert ctx.lib.zh_saw_env_patch_default(C.byref(patch)) == 0 and ctx.lib.zh_saw_env_patch_default(None) == abi.ZH_ERR_INVALID
    assert [round(x, 6) for x in (patch.color, patch.attack, patch.decay, patch.release, patch.sustain_volume)] == [0.0, 0.025, 0.1, 0.15, 0.5]
    ctx.sync()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and m.state().tobytes() == state
    m.close()
