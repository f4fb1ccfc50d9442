"""GPU: the two-source example's voice -- zh_dual_paint[_spans] (k_dual_spans) -- against tests/two_reference.py: the oracle's
TriSawOsc and Envelope per voice and per sub-span under zero, multiply and addScalarInto, as examples/example_two.zig:109-138, :153
runs them.  Everything on bits: the uint32 views of both output images and the six state words after every buffer; any NaN equals
any NaN (by position).  At most 96 frames; sub-spans of 0, 1, 7, 8 and 9 frames around the 8-frame chunk and one of 30, in every
voice's own order, a frame or two apart or adjacent; 1, 63, 64, 65 and 130 voices."""
import itertools

import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import two_reference as tr
from tests import util

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 4000.0                                        # the oscillator paints 0 .. SR / 8 = 500 Hz
ROWS, SPAN = 96, (3, 93)
LENGTHS = (0, 1, 7, 8, 9, 30)
K = len(LENGTHS)
VOICES = [1, 63, 64, 65, 130]
PATCH = (0.002, 0.003, 0.004, 0.25)                # stages of 8, 12 and 16 frames: they end, and flip, inside the sub-spans


def tables(V, seed, hostile=False):
    """six sub-spans per voice, lengths 0, 1, 7, 8, 9 and 30 in the voice's own order, the first at 3 .. 6, each 0 to 2 frames after
    the last; voice v % 7 == 6 has four only.  freq, color and note_on per sub-span; note_id_changed mostly follows a note-on.
    `hostile`: frequencies below 0 and above SR / 8 (the oscillator paints nothing), colours that are NaN, 0 and 1"""
    rng = np.random.default_rng(seed)
    perms = list(itertools.permutations(range(K)))
    tb = {"count": np.zeros(V, np.uint32), "start": np.zeros((K, V), np.uint32), "end": np.zeros((K, V), np.uint32),
          "nic": np.zeros((K, V), np.uint8), "freq": rng.uniform(40.0, 480.0, (K, V)).astype(f32),
          "color": rng.uniform(0.0, 1.0, (K, V)).astype(f32), "note_on": (rng.random((K, V)) < 0.6).astype(np.uint32)}
    for v in range(V):
        pos = SPAN[0] + v % 4
        n = 4 if v % 7 == 6 else K
        for k, i in enumerate(perms[(v * 37) % len(perms)][:n]):
            pos += (v + k) % 3 if k else 0
            tb["start"][k, v], tb["end"][k, v] = pos, pos + LENGTHS[i]
            pos += LENGTHS[i]
        assert pos <= SPAN[1]
        tb["count"][v] = n
    tb["nic"][:] = (tb["note_on"] != 0) & (rng.random((K, V)) < 0.7)
    if hostile:
        tb["freq"][:] = rng.choice(np.array([-1.0, -220.0, 499.0, 500.0, 501.0, 600.0, 4000.0, 220.0, 110.0], f32), (K, V))
        tb["color"][:] = rng.choice(np.array([np.nan, 0.0, 1.0, 0.25, 0.75, 0.5, -0.5, 1.5], f32), (K, V))
    return tb


def base_image(V, seed, minus_zero=True):
    img = np.random.default_rng(seed).uniform(-1.0, 1.0, (V, ROWS)).astype(f32)
    if minus_zero:
        img[:, ::5] = -0.0
    return img


def _table(m, tb, names=tr.FIELDS):
    values = {n: ((None, tb[n]) if n == "note_on" else (tb[n], None)) for n in names}
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], values if names else None)


def _voices(oracle, V):
    return [tr.Voice(oracle) for _ in range(V)]


def _words(m):
    st = m.state()
    u = lambda a: np.ascontiguousarray(a).view(np.uint32) if a.dtype == f32 else a.astype(np.uint32)
    cols = [st["osc"]["cnt"], st["osc"]["t"], st["env"]["state"], st["env"]["t"], st["env"]["last_value"], st["env"]["start"]]
    return np.stack([u(np.ascontiguousarray(c)) for c in cols], 1).tolist()


def _check(m, outs, refs, vs, what):
    for name, out, ref in zip(("audio", "sync"), outs, refs):
        if out is not None:
            got = util.from_image(out)
            assert hc.same_f32(got, ref), (what, name, hc.first_difference(got, ref))
    assert _words(m) == [v.words() for v in vs], what + " state"


@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("o1", [True, False], ids=["sync", "no_sync"])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_equals_the_model(ctx, oracle, V, zero_first, o1):
    """two consecutive buffers with carried state (the round trip of the state across two paints), every field from span arrays;
    rows outside [3, 93) and -- without zero_first -- frames no sub-span covers keep their bits, -0.0 included"""
    from zang_amd import modules as mod, zang
    m = mod.Dual(V, ctx)
    vs = _voices(oracle, V)
    patch = m.Patch(*PATCH)
    for b in range(2):
        tb = tables(V, 1000 * V + b)
        base, sbase = base_image(V, 77 + V + b), base_image(V, 177 + V + b)
        ref, sref = base.copy(), sbase.copy()
        tr.paint_spans(oracle, vs, tb, ref, sref if o1 else None, SPAN, SR, zero_first, PATCH)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*SPAN), [out, sync] if o1 else [out], None, m.Params(SR, patch=patch), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_dual_spans"], ctx.last_form()
        _check(m, (out, sync), (ref, sref), vs, f"V={V} buffer {b}")    # an unpainted sync image keeps every bit
        assert float(np.abs(ref[:, SPAN[0]:SPAN[1]]).max()) > 0.05 and not hc.same_f32(ref, base)
        if not zero_first:                                             # uncovered frames inside the span: -0.0 stays -0.0
            v = V - 1
            gap = [i for i in range(SPAN[0], SPAN[1]) if not any(tb["start"][k, v] <= i < tb["end"][k, v] for k in range(int(tb["count"][v])))]
            assert gap and np.array_equal(ref[v, gap].view(np.uint32), base[v, gap].view(np.uint32))
    m.close()


@pytest.mark.parametrize("patch", [PATCH, None], ids=["short_stages", "the_examples"])
def test_hostile_fields(ctx, oracle, patch):
    """frequencies below 0 and above SR / 8 (the oscillator paints nothing: the zeroed temp still goes through the multiply-add, so
    -0.0 becomes +0.0 inside a sub-span), NaN and out-of-range colours, note_on flipping inside a release"""
    from zang_amd import modules as mod, zang
    V = 130
    m = mod.Dual(V, ctx)
    vs = _voices(oracle, V)
    for b in range(2):
        tb = tables(V, 606 + b, hostile=True)
        tb["note_on"][:, 1] = 0                                        # voice 1 never had a note: the envelope stays idle
        tb["freq"][:, 1] = 600.0                                       # ... and its oscillator is out of range throughout
        tb["note_on"][:, 2] = [1, 0, 1, 0, 1, 0]                       # voice 2: off and on again, stage after stage
        tb["nic"][:, 2] = [1, 0, 0, 0, 1, 0]
        base, sbase = base_image(V, 12 + b), base_image(V, 13 + b)
        ref, sref = base.copy(), sbase.copy()
        tr.paint_spans(oracle, vs, tb, ref, sref, SPAN, SR, False, patch)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*SPAN), [out, sync], None, m.Params(SR, patch=None if patch is None else m.Patch(*patch)), _table(m, tb))
        ctx.sync()
        _check(m, (out, sync), (ref, sref), vs, f"hostile, buffer {b}")
        k = int(np.argmax(tb["end"][:, 1] - tb["start"][:, 1]))        # voice 1's sub-span of 30 frames
        s, e = int(tb["start"][k, 1]), int(tb["end"][k, 1])
        inside = np.arange(s, e)[np.arange(s, e) % 5 == 0]
        assert len(inside) >= 5 and (ref[1, inside].view(np.uint32) == 0).all() and vs[1].words()[0] == 0
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_plain_paint_equals_the_model_and_the_span_form(ctx, oracle, V):
    """zh_dual_paint: V voices with their own freq, color and note_on over spans of 1, 9 and 30 frames (ADD, ZERO_FIRST, ADD), with
    and without the sync image, carried state and note_id_changed on, off, on == the model == the span form over one full sub-span
    per voice"""
    from zang_amd import modules as mod, zang
    ms = [mod.Dual(V, ctx) for _ in range(2)]
    vs = _voices(oracle, V)
    rng = np.random.default_rng(V)
    pos = SPAN[0]
    for b, length in enumerate((1, 9, 30)):
        S, E = pos, pos + length
        pos = E
        nic, zf, o1 = b != 1, b == 1, b != 2
        tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
              "nic": np.full((1, V), nic, np.uint8), "freq": rng.uniform(40.0, 480.0, (1, V)).astype(f32),
              "color": rng.uniform(0.0, 1.0, (1, V)).astype(f32), "note_on": (np.arange(V)[None, :] % 3 != b).astype(np.uint32)}
        base, sbase = base_image(V, 31 + V + b), base_image(V, 41 + V + b)
        ref, sref = base.copy(), sbase.copy()
        tr.paint_spans(oracle, vs, tb, ref, sref if o1 else None, (S, E), SR, zf, PATCH)
        outs = [(util.to_image(base), util.to_image(sbase)) for _ in range(2)]
        patch = ms[0].Patch(*PATCH)
        params = ms[0].Params(SR, util.dev(tb["freq"][0]), util.dev(tb["color"][0]), util.dev(tb["note_on"][0].astype(np.uint8)), patch)
        ms[0].paint(zang.Span(S, E), list(outs[0]) if o1 else [outs[0][0]], [], nic, params, zero_first=zf)
        ms[1].paint_spans(zang.Span(S, E), list(outs[1]) if o1 else [outs[1][0]], None, ms[1].Params(SR, patch=patch), _table(ms[1], tb), zero_first=zf)
        ctx.sync()
        for i, what in enumerate(("plain", "one sub-span")):
            _check(ms[i], outs[i], (ref, sref), vs, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


@pytest.mark.parametrize("how", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, how):
    from zang_amd import modules as mod, zang
    V = 65
    tb = tables(V, 4242)
    m = mod.Dual(V, ctx)
    vs = _voices(oracle, V)
    rng = np.random.default_rng(5)
    patch = m.Patch(*PATCH)
    if how == "broadcast":
        dflt, params, names = {"freq": f32(330.0), "color": f32(0.3), "note_on": 1}, m.Params(SR, 330.0, 0.3, True, patch), ()
    else:
        dflt = {"freq": rng.uniform(40.0, 480.0, V).astype(f32), "color": rng.uniform(0.0, 1.0, V).astype(f32),
                "note_on": (np.arange(V) % 3 != 0).astype(np.uint32)}
        params = m.Params(SR, util.dev(dflt["freq"]), util.dev(dflt["color"]), util.dev(dflt["note_on"].astype(np.uint8)), patch)
        names = () if how == "per_voice" else ("color",)
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base, sbase = base_image(V, 3), base_image(V, 4)
    ref, sref = base.copy(), sbase.copy()
    tr.paint_spans(oracle, vs, lean, ref, sref, SPAN, SR, False, PATCH, dflt=dflt)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*SPAN), [out, sync], None, params, _table(m, tb, names))
    ctx.sync()
    _check(m, (out, sync), (ref, sref), vs, how)
    m.close()


def test_state_round_trip(ctx, oracle):
    from zang_amd import modules as mod, zang
    V = 3
    m = mod.Dual(V, ctx)
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
          "nic": np.zeros((1, V), np.uint8), "freq": np.full((1, V), 220.0, f32), "color": np.full((1, V), 0.7, f32), "note_on": on[None, :]}
    base, sbase = base_image(V, 8), base_image(V, 9)
    ref, sref = base.copy(), sbase.copy()
    tr.paint_spans(oracle, vs, tb, ref, sref, SPAN, SR, False, PATCH)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint(zang.Span(*SPAN), [out, sync], [], False, m.Params(SR, 220.0, 0.7, util.dev(on.astype(np.uint8)), m.Patch(*PATCH)))
    ctx.sync()
    _check(m, (out, sync), (ref, sref), vs, "from a set state")
    m.close()


def test_refusals(ctx):
    import ctypes as C
    import torch
    from zang_amd import abi, modules as mod, zang
    V = 8
    tb = tables(V, 1)
    m = mod.Dual(V, ctx)
    out, sync = ctx.image(ROWS, V, fill=0.25), ctx.image(ROWS, V, fill=0.5)
    before, state = out.clone(), m.state().tobytes()
    span, good = zang.Span(*SPAN), m.Params(SR)
    assert m._paint_spans(span, [out, sync], None, good, _table(m, tb), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_spans(span, [out[:50], sync], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID       # too few rows
    assert m._paint_spans(span, [out, sync[:50]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID       # ... of outputs[1]
    wide, marker = ctx.image(ROWS, 2 * V, fill=0.5), ctx.last_form()    # outputs[1] shares a float with outputs[0]: refused, no launch
    assert m._paint_spans(span, [out, out], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID                  # the same image
    assert m._paint_spans(span, [wide[:, :V], wide[:, V - 1:2 * V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID   # one column in common
    assert ctx.last_form() == marker
    assert m._paint_spans(span, [out[:, :V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID       # too few voices
    with pytest.raises(abi.ZangHipError):
        m.paint(span, [out[:50]], [], False, good)
    paint, paint_spans = ctx.lib.zh_dual_paint, ctx.lib.zh_dual_paint_spans
    outs, cp = m._outputs([out, sync]), m._cparams(good)
    ctb, sp = _table(m, tb).device(ctx.device, list(tr.FIELDS))
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID          # end < start
    assert paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), None, 0) == abi.ZH_ERR_INVALID
    assert paint(None, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, 0) == abi.ZH_ERR_INVALID
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.DUAL_SPAN_NOTE_ON] = abi.ScriptSpanParam(sp[abi.DUAL_SPAN_FREQ].f, None)                                    # `f` on a u-only field
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.DUAL_SPAN_COLOR] = abi.ScriptSpanParam(None, sp[abi.DUAL_SPAN_NOTE_ON].u)                                   # `u` on an f-only field
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    patch = abi.DualPatch()
    assert ctx.lib.zh_dual_patch_default(C.byref(patch)) == 0 and ctx.lib.zh_dual_patch_default(None) == abi.ZH_ERR_INVALID
    assert [round(x, 6) for x in (patch.attack, patch.decay, patch.release, patch.sustain_volume)] == [0.025, 0.1, 1.0, 0.5]
    assert (abi.DUAL_SPAN_FREQ, abi.DUAL_SPAN_COLOR, abi.DUAL_SPAN_NOTE_ON, abi.DUAL_SPAN_FIELDS) == (0, 1, 2, 3)
    ctx.sync()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and m.state().tobytes() == state
    m.close()

