"""GPU: the controlled phase-modulation voice -- zh_pmctl_paint, zh_pmctl_paint_spans (k_pmctl_spans) and zh_pmctl_paint_controlled
(k_pmctl_controlled) -- against tests/mouse_reference.py: examples/example_mouse.zig and the PhaseModOscillator of
examples/modules.zig restated over the oracle's Portamento, SineOsc and Envelope.  Everything on bits: the uint32 views of the
output image, of the carried temp image and of the twelve state words after every buffer; any NaN equals any NaN (by position).
Shapes and streams: tests/mouse_cases.py (images of 100 rows; buffers of 1, 7 and 96 frames; 1, 63, 64, 65 and 130 voices)."""
import ctypes as C

import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import mouse_cases as mc
from tests import mouse_reference as mr
from tests import util

pytestmark = pytest.mark.gpu
f32 = np.float32


def _patch(m, p=mc.PATCH):
    return m.Patch(p.ctl_curve, p.ctl_glide, p.attack, p.decay, p.release, p.sustain_volume)


def _notes(m, tb, names=("freq", "note_on")):
    values = {n: ((None, tb[n]) if n == "note_on" else (tb[n], None)) for n in names}
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], values if names else None)


def _ctl(m, tb, scale):
    return m.Control(m.control_table(tb["count"], tb["start"], tb["end"], tb["nic"], tb["value"], tb["note_on"]), scale)


def _relative(V, how):
    """-> (the model's relative and scales, the device's)"""
    if how != "mixed":
        rel = how == "on"
        return (rel, mc.SCALES[rel]), (rel, mc.SCALES[rel])
    rel = np.arange(V) % 2 == 0
    rs = np.where(rel, f32(mc.SCALES[True][0]), f32(mc.SCALES[False][0])).astype(f32)
    return (rel, (rs, mc.SCALES[True][1])), (util.dev(rel.astype(np.uint8)), (util.dev(rs), mc.SCALES[True][1]))


def _check(m, out, ref, vs, what, stale=None, stale_ref=None):
    got = util.from_image(out)
    assert hc.same_f32(got, ref), (what, "audio", hc.first_difference(got, ref))
    if stale is not None:
        got = util.from_image(stale)
        assert hc.same_f32(got, stale_ref), (what, "carried temp", hc.first_difference(got, stale_ref))
    assert mr.same_words(mr.struct_state(m.state()), mr.state_words(vs)), what + " state"


COMBOS = [(False, "mixed", True), (True, "on", False), (True, "off", True), (False, "on", True), (False, "off", False), (True, "mixed", False)]


@pytest.mark.parametrize("V", mc.VOICES)
@pytest.mark.parametrize("F", [1, 7, 96])
@pytest.mark.parametrize("zero_first,how,carried", COMBOS, ids=[f"{'zf' if z else 'add'}-{h}-{'temp' if c else 'notemp'}" for z, h, c in COMBOS])
def test_paint_controlled_equals_the_model(ctx, oracle, V, F, zero_first, how, carried):
    """three consecutive buffers of random streams per voice (tests/mouse_cases.py: a stream without rows, a control that starts
    late, rows that end together in two and in three streams, empty rows, an out-of-order row in one stream), state and temp
    carried; rows outside the span and -- without zero_first -- frames no note covers keep their bits"""
    from zang_amd import modules as mod, zang
    m = mod.PMCtl(V, ctx)
    vs = [mr.Voice(oracle) for _ in range(V)]
    (rel_m, scales_m), (rel_d, scales_d) = _relative(V, how)
    stale_ref = mc.base_image(V, 5 + V, minus_zero=False) if carried else None
    stale = util.to_image(stale_ref) if carried else None
    span = mc.SPANS[F]
    changed = False
    for b in range(3):
        tbs = mc.streams(V, F, 10 * V + F + b)
        base = mc.base_image(V, 77 + V + b)
        ref = base.copy()
        mr.paint_controlled(oracle, vs, tbs, ref, stale_ref, span, mc.SR, zero_first, rel_m, scales_m, mc.PATCH)
        out = util.to_image(base)
        m.paint_controlled(zang.Span(*span), [out], [None, stale, None] if carried else None, m.Params(mc.SR, relative=rel_d, patch=_patch(m)),
                           _notes(m, tbs[mr.NOTES]), _ctl(m, tbs[mr.RATIO], scales_d[0]), _ctl(m, tbs[mr.MULT], scales_d[1]), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_pmctl_controlled"], ctx.last_form()
        _check(m, out, ref, vs, f"V={V} F={F} buffer {b}", stale, stale_ref)
        changed = changed or not hc.same_f32(ref, base)
    assert changed or F < 96                                           # the streams make sound
    m.close()


def _compose(ctx, m, portas, span, tbs, out, temps, params, scales, zero_first):
    """the composition a caller has without the fused form: each control's Portamento painted row by row into a zeroed image
    (zh_portamento_paint; the rows' boundaries are the same for every voice, values, note_on and note_id_changed per voice), then
    zh_pmctl_paint_spans with the two images as buffers"""
    from zang_amd import zang
    imgs = []
    for tb, porta, scale in zip(tbs[1:], portas, scales):
        img = ctx.image(mc.ROWS, m.n_voices, fill=0.0)
        for k in range(int(tb["count"][0])):
            with np.errstate(all="ignore"):
                goal = (tb["value"][k] * f32(scale)).astype(f32)
            curve = zang.PaintCurve._mk(int(params.patch.ctl_curve), float(params.patch.ctl_glide))
            porta.paint(zang.Span(int(tb["start"][k, 0]), int(tb["end"][k, 0])), [img], [], util.dev(tb["nic"][k]),
                        porta.Params(params.sample_rate, curve, util.dev(goal), util.dev(tb["note_on"][k].astype(np.uint8)), True))
        imgs.append(img)
    m.paint_spans(zang.Span(*span), [out], temps, params, _notes(m, tbs[mr.NOTES]), zang.buffer(imgs[0]), zang.buffer(imgs[1]), zero_first=zero_first)


def _composed_state(m, portas):
    st = m.state()
    for name, p in zip(("ratio", "multiplier"), portas):
        st[name] = p.state()
    return mr.struct_state(st)


@pytest.mark.parametrize("V", [65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_paint_controlled_equals_the_composition_on_the_device(ctx, V, zero_first):
    """three buffers; the fused launch against Portamento paints into zeroed images + the span paint with buffer cobs: the output,
    the carried temp and get_state (the composition's two Portamento states are its Portamento modules')"""
    from zang_amd import modules as mod, zang
    fused, comp, portas = mod.PMCtl(V, ctx), mod.PMCtl(V, ctx), [mod.Portamento(V, ctx) for _ in range(2)]
    stales = [util.to_image(np.zeros((V, mc.ROWS), f32)) for _ in range(2)]
    params = fused.Params(mc.SR, relative=True, patch=_patch(fused))
    span = mc.SPANS[96]
    for b in range(3):
        tbs = [mc.streams(V, 96, 300 + V + b)[mr.NOTES]] + mc.uniform_controls(V, 96, 400 + V + b)
        base = mc.base_image(V, 7 + b)
        outs = [util.to_image(base) for _ in range(2)]
        fused.paint_controlled(zang.Span(*span), [outs[0]], [None, stales[0], None], params, _notes(fused, tbs[0]),
                               _ctl(fused, tbs[1], mc.SCALES[True][0]), _ctl(fused, tbs[2], mc.SCALES[True][1]), zero_first=zero_first)
        _compose(ctx, comp, portas, span, tbs, outs[1], [None, stales[1], None], params, mc.SCALES[True], zero_first)
        ctx.sync()
        a, c = util.from_image(outs[0]), util.from_image(outs[1])
        assert hc.same_f32(a, c), (b, hc.first_difference(a, c))
        assert not hc.same_f32(a, base)
        assert hc.same_f32(util.from_image(stales[0]), util.from_image(stales[1]))
        assert mr.same_words(mr.struct_state(fused.state()), _composed_state(comp, portas)), f"buffer {b} state"
    for o in [fused, comp] + portas:
        o.close()


def _cob(kind, V, seed, lo, hi):
    """-> (the model's cob, the device's): "const", "per_voice" or "buffer" """
    from zang_amd import zang
    rng = np.random.default_rng(seed)
    if kind == "const":
        x = f32(rng.uniform(lo, hi))
        return ("c", x), zang.constant(float(x))
    if kind == "per_voice":
        x = rng.uniform(lo, hi, V).astype(f32)
        return ("c", x), zang.constant(util.dev(x))
    img = rng.uniform(lo, hi, (V, mc.ROWS)).astype(f32)
    return ("b", img), zang.buffer(util.to_image(img))


@pytest.mark.parametrize("V", [1, 65, 130])
@pytest.mark.parametrize("relative", [True, False], ids=["relative", "absolute"])
@pytest.mark.parametrize("rk,mk", [("const", "per_voice"), ("const", "buffer"), ("buffer", "const"), ("buffer", "buffer")])
def test_paint_spans_equals_the_model(ctx, oracle, V, relative, rk, mk):
    """the four constant / buffer combinations over two buffers of random note tables, the temp carried (it is read in the
    relative / buffer branch only and written in every branch)"""
    from zang_amd import modules as mod, zang
    m = mod.PMCtl(V, ctx)
    vs = [mr.Voice(oracle) for _ in range(V)]
    lo, hi = (0.25, 4.0) if relative else (20.0, 480.0)
    (rm, rd), (mm, md) = _cob(rk, V, 1, lo, hi), _cob(mk, V, 2, 0.0, 2.0)
    stale_ref = mc.base_image(V, 9, minus_zero=False)
    stale = util.to_image(stale_ref)
    span = mc.SPANS[96]
    for b in range(2):
        tb = mc.streams(V, 96, 50 + V + b)[mr.NOTES]
        base = mc.base_image(V, 21 + b)
        ref = base.copy()
        mr.paint_spans(oracle, vs, tb, ref, stale_ref, span, mc.SR, b == 1, relative, rm, mm, mc.PATCH)
        out = util.to_image(base)
        m.paint_spans(zang.Span(*span), [out], [None, stale, None], m.Params(mc.SR, relative=relative, patch=_patch(m)), _notes(m, tb), rd, md,
                      zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_pmctl_spans"], ctx.last_form()
        _check(m, out, ref, vs, f"buffer {b}", stale, stale_ref)
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_plain_paint_equals_the_model_and_the_span_form(ctx, oracle, V):
    """zh_pmctl_paint over spans of 1, 9 and 30 frames (ADD, ZERO_FIRST, ADD) with per-voice freq, note_on and relative, a buffer
    ratio and a per-voice multiplier, note_id_changed on, off, on == the model == the span form over one full sub-span per voice;
    fields without a span array come from the params"""
    from zang_amd import modules as mod, zang
    ms = [mod.PMCtl(V, ctx) for _ in range(2)]
    vs = [mr.Voice(oracle) for _ in range(V)]
    rng = np.random.default_rng(V)
    (rm, rd), (mm, md) = _cob("buffer", V, 3, 0.25, 4.0), _cob("per_voice", V, 4, 0.0, 2.0)
    rel = np.arange(V) % 3 != 0
    stale_ref = np.zeros((V, mc.ROWS), f32)
    stales = [util.to_image(stale_ref) for _ in range(2)]
    pos = 3
    for b, length in enumerate((1, 9, 30)):
        S, E = pos, pos + length
        pos = E
        nic, zf = b != 1, b == 1
        freq, on = rng.uniform(40.0, 480.0, V).astype(f32), (np.arange(V) % 3 != b).astype(np.uint32)
        tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
              "nic": np.full((1, V), nic, np.uint8), "freq": None, "note_on": None}
        base = mc.base_image(V, 31 + V + b)
        ref = base.copy()
        mr.paint_spans(oracle, vs, tb, ref, stale_ref, (S, E), mc.SR, zf, rel, rm, mm, mc.PATCH, dflt={"freq": freq, "note_on": on})
        outs = [util.to_image(base) for _ in range(2)]
        params = ms[0].Params(mc.SR, util.dev(freq), util.dev(on.astype(np.uint8)), util.dev(rel.astype(np.uint8)), _patch(ms[0]))
        ms[0].paint(zang.Span(S, E), [outs[0]], [None, stales[0], None], nic, params, rd, md, zero_first=zf)
        ms[1].paint_spans(zang.Span(S, E), [outs[1]], [None, stales[1], None], params, _notes(ms[1], tb, ()), rd, md, zero_first=zf)
        ctx.sync()
        for i, what in enumerate(("plain", "one sub-span")):
            _check(ms[i], outs[i], ref, vs, f"V={V} paint {b} {what}", stales[i], stale_ref)
    for m in ms:
        m.close()


@pytest.mark.parametrize("V", [3, 130])
def test_constants_of_one_are_the_pinned_pmosc_voice(ctx, V):
    """ratio = multiplier = 1.0, relative on, the same release: zh_pmctl_paint == zh_pmosc_paint, output and state, over three
    paints (note on, held, released)"""
    from zang_amd import modules as mod, zang
    rel = 0.004
    a, b = mod.PMCtl(V, ctx), mod.PMOscInstrument(V, rel, ctx)
    freq = util.dev(np.random.default_rng(V).uniform(40.0, 480.0, V).astype(f32))
    patch = a.Patch(release=rel)                                       # attack, decay and sustain are zh_pmosc's constants
    pos = 2
    for nic, on, length in ((True, True, 40), (False, True, 7), (False, False, 49)):
        span = zang.Span(pos, pos + length)
        pos += length
        base = mc.base_image(V, pos)
        outs = [util.to_image(base) for _ in range(2)]
        a.paint(span, [outs[0]], None, nic, a.Params(mc.SR, freq, on, True, patch), zang.constant(1.0), zang.constant(1.0))
        b.paint(span, [outs[1]], [], nic, b.Params(mc.SR, freq, on))
        ctx.sync()
        x, y = util.from_image(outs[0]), util.from_image(outs[1])
        assert hc.same_f32(x, y), hc.first_difference(x, y)
        assert not hc.same_f32(x, base)
        sa, sb = a.state(), b.state()
        for obj, f in (("carrier", "t"), ("modulator", "t"), ("env", "state"), ("env", "t"), ("env", "last_value"), ("env", "start")):
            assert sa[obj][f].tobytes() == sb[obj][f].tobytes(), (obj, f)
    a.close(); b.close()


def test_the_stale_temp(ctx, oracle):
    """two buffers of the held note (tests/mouse_cases.py held_note) in relative mode: with the image carried == the persisting
    model; with NULL == the zeroing model; the first buffers are equal (the image starts as zeros inside the span) and the second
    DIFFER; the image afterwards holds the envelope, and frames outside every note sub-span keep what they held"""
    from zang_amd import modules as mod, zang
    V, span = 65, mc.SPANS[96]
    S, E = span
    results = {}
    for carried in (True, False):
        m = mod.PMCtl(V, ctx)
        vs = [mr.Voice(oracle) for _ in range(V)]
        stale_ref = snap = None
        if carried:
            stale_ref = mc.base_image(V, 3, minus_zero=False)
            stale_ref[:, S:E] = 0.0
            outside = stale_ref.copy()
        stale = util.to_image(stale_ref) if carried else None
        for b in range(2):
            tbs = mc.held_note(V, b)
            if b == 1:                                                 # voice 1's row ends at frame 40: no note after it
                tbs[mr.NOTES]["end"][0, 1] = 40
            ref = np.zeros((V, mc.ROWS), f32)
            mr.paint_controlled(oracle, vs, tbs, ref, stale_ref, span, mc.SR, True, True, mc.SCALES[True], mc.PATCH)
            out = util.to_image(np.zeros((V, mc.ROWS), f32))
            m.paint_controlled(zang.Span(*span), [out], [None, stale, None] if carried else None, m.Params(mc.SR, relative=True, patch=_patch(m)),
                               _notes(m, tbs[mr.NOTES]), _ctl(m, tbs[mr.RATIO], mc.SCALES[True][0]), _ctl(m, tbs[mr.MULT], mc.SCALES[True][1]),
                               zero_first=True)
            ctx.sync()
            _check(m, out, ref, vs, f"carried={carried} buffer {b}", stale, stale_ref)
            results[carried, b] = util.from_image(out)
            if carried and b == 0:
                snap = util.from_image(stale)
        if carried:
            got = util.from_image(stale)
            for rows in (slice(0, S), slice(E, mc.ROWS)):                                                    # rows outside the span
                assert np.array_equal(got[:, rows].view(np.uint32), outside[:, rows].view(np.uint32))
            assert np.all(snap[0, S:S + 4] > 0.0) and np.all(snap[0, S:S + 4] < 1.0)                         # buffer 0: the attack
            assert np.all(got[0, S:E] == f32(mc.PATCH.sustain_volume))                                       # buffer 1: held at sustain
            assert np.array_equal(got[1, 40:E].view(np.uint32), snap[1, 40:E].view(np.uint32))               # no note there: kept
        m.close()
    assert hc.same_f32(results[True, 0], results[False, 0])
    assert not hc.same_f32(results[True, 1], results[False, 1])


HOSTILE_PATCHES = {"the_tests": {}, "glide_0": {"ctl_glide": 0.0}, "glide_nan": {"ctl_glide": float("nan")}, "glide_neg": {"ctl_glide": -1.0},
                   "attack_inf": {"attack": float("inf")}, "sustain_nan": {"sustain_volume": float("nan")}, "release_0": {"release": 0.0},
                   "instantaneous": {"ctl_curve": 0}, "squared": {"ctl_curve": 2}, "cubed": {"ctl_curve": 3}}


@pytest.mark.parametrize("name", list(HOSTILE_PATCHES))
def test_hostile_fields_and_patches_do_what_the_composition_does(ctx, name):
    """tests/hostile_cases.py's values (NaN, infinities, zeros, denormals, huge, negative) as note frequencies, control values and
    scales, one hostile patch field at a time, and a hostile sample rate once: the fused launch == the composition, on bits"""
    from dataclasses import replace
    from zang_amd import modules as mod, zang
    V, span = 130, mc.SPANS[96]
    p = replace(mc.PATCH, **HOSTILE_PATCHES[name])
    sr = 0.0 if name == "release_0" else mc.SR
    fused, comp, portas = mod.PMCtl(V, ctx), mod.PMCtl(V, ctx), [mod.Portamento(V, ctx) for _ in range(2)]
    stales = [util.to_image(np.zeros((V, mc.ROWS), f32)) for _ in range(2)]
    params = fused.Params(sr, relative=True, patch=_patch(fused, p))
    rng = np.random.default_rng(len(name))
    hostile = np.array(hc.HOSTILE, f32)
    scales = (f32(4.0), f32(np.inf) if name == "squared" else f32(2.0))
    for b in range(2):
        tbs = [mc.streams(V, 96, 900 + b)[mr.NOTES]] + mc.uniform_controls(V, 96, 950 + b)
        for tb, field in zip(tbs, ("freq", "value", "value")):
            pick = rng.random(tb[field].shape) < 0.3
            tb[field][pick] = rng.choice(hostile, int(pick.sum()))
        base = mc.base_image(V, 17 + b)
        outs = [util.to_image(base) for _ in range(2)]
        fused.paint_controlled(zang.Span(*span), [outs[0]], [None, stales[0], None], params, _notes(fused, tbs[0]),
                               _ctl(fused, tbs[1], float(scales[0])), _ctl(fused, tbs[2], float(scales[1])))
        _compose(ctx, comp, portas, span, tbs, outs[1], [None, stales[1], None], params, scales, False)
        ctx.sync()
        a, c = util.from_image(outs[0]), util.from_image(outs[1])
        assert hc.same_f32(a, c), (b, hc.first_difference(a, c))
        assert hc.same_f32(util.from_image(stales[0]), util.from_image(stales[1]))
        assert mr.same_words(mr.struct_state(fused.state()), _composed_state(comp, portas)), f"buffer {b} state"
    for o in [fused, comp] + portas:
        o.close()


def test_state_round_trip(ctx, oracle):
    from zang_amd import modules as mod, zang
    V = 3
    m = mod.PMCtl(V, ctx)
    st = m.state()
    assert st.tobytes() == bytes(st.nbytes)                            # create == init(): every word zero
    st["ratio"]["t"][:] = (0.5, 1.0, 0.0); st["ratio"]["last_value"][:] = (1.5, 2.0, 0.25); st["ratio"]["start"][:] = (1.0, 0.0, 0.25)
    st["multiplier"]["t"][:] = (0.25, 0.0, 1.0); st["multiplier"]["last_value"][:] = (0.5, 0.0, 1.25); st["multiplier"]["start"][:] = (0.0, 0.0, 1.0)
    st["carrier"]["t"][:] = (0.25, -3.5, 100.75); st["modulator"]["t"][:] = (0.5, 0.125, -0.75)
    st["env"]["state"][:] = (1, 3, 4)                                  # attack, sustain, release
    st["env"]["t"][:] = (0.5, 0.0, 0.25); st["env"]["last_value"][:] = (0.75, 0.25, 0.2); st["env"]["start"][:] = (0.1, 0.25, 0.25)
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    vs = [mr.Voice(oracle) for _ in range(V)]
    for v in range(V):
        vs[v].load(st, v)
    assert mr.same_words(mr.struct_state(st), mr.state_words(vs))
    tbs = mc.held_note(V, 1)
    tbs[mr.NOTES]["note_on"][0] = (1, 1, 0)
    base = mc.base_image(V, 8)
    ref = base.copy()
    mr.paint_controlled(oracle, vs, tbs, ref, None, mc.SPANS[96], mc.SR, False, True, mc.SCALES[True], mc.PATCH)
    out = util.to_image(base)
    m.paint_controlled(zang.Span(*mc.SPANS[96]), [out], None, m.Params(mc.SR, patch=_patch(m)), _notes(m, tbs[mr.NOTES]),
                       _ctl(m, tbs[mr.RATIO], mc.SCALES[True][0]), _ctl(m, tbs[mr.MULT], mc.SCALES[True][1]))
    ctx.sync()
    _check(m, out, ref, vs, "from a set state")
    m.close()


def test_refusals(ctx):
    import torch
    from zang_amd import abi, modules as mod, zang
    V = 8
    tbs = mc.streams(V, 96, 1)
    m = mod.PMCtl(V, ctx)
    out, temp, img = ctx.image(mc.ROWS, V, fill=0.25), ctx.image(mc.ROWS, V, fill=0.5), ctx.image(mc.ROWS, V, fill=1.0)
    before, state = out.clone(), m.state().tobytes()
    span, good = zang.Span(*mc.SPANS[96]), m.Params(mc.SR)
    notes, rc, mc_ = _notes(m, tbs[0]), _ctl(m, tbs[1], 4.0), _ctl(m, tbs[2], 2.0)
    one, buf = zang.constant(1.0), zang.buffer(img)
    INV, UNS = abi.ZH_ERR_INVALID, abi.ZH_ERR_UNSUPPORTED
    # the three paints: tolerant, short images, a short temp
    assert m._paint_rc(span, [out], None, False, good, one, one, abi.PAINT_TOLERANT) == UNS
    assert m._paint_spans(span, [out], None, good, notes, abi.PAINT_TOLERANT, None, one, buf) == UNS
    assert m._paint_controlled(span, [out], None, good, notes, rc, mc_, abi.PAINT_TOLERANT) == UNS
    assert m._paint_rc(span, [out[:50]], None, False, good, one, one, 0) == INV
    assert m._paint_spans(span, [out[:, :V - 1]], None, good, notes, 0, None, one, one) == INV
    assert m._paint_controlled(span, [out[:50]], None, good, notes, rc, mc_, 0) == INV
    assert m._paint_controlled(span, [out], [None, temp[:50], None], good, notes, rc, mc_, 0) == INV
    assert m._paint_rc(span, [out], [None, temp[:, :V - 1], None], False, good, one, one, 0) == INV
    # cobs: an unknown tag, a buffer that is too small, NULL
    bad_tag = zang.constant(1.0); bad_tag.tag = 7
    assert m._paint_rc(span, [out], None, False, good, bad_tag, one, 0) == INV
    assert m._paint_spans(span, [out], None, good, notes, 0, None, one, bad_tag) == INV
    assert m._paint_rc(span, [out], None, False, good, zang.buffer(img[:50]), one, 0) == INV
    assert m._paint_spans(span, [out], None, good, notes, 0, None, one, zang.buffer(img[:, :V - 1])) == INV
    paint, paint_spans, controlled = ctx.lib.zh_pmctl_paint, ctx.lib.zh_pmctl_paint_spans, ctx.lib.zh_pmctl_paint_controlled
    outs, cp = mod._bufarray([out]), m._cparams(good)
    ctb, sp = notes.device(ctx.device, ["freq", "note_on"])
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), None, C.byref(one), 0) == INV
    assert paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), C.byref(one), C.byref(one), 0) == INV
    assert paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), C.byref(one), C.byref(one), 0) == INV
    assert paint(m.handle, span.start, span.end, outs, None, abi.Bool(), None, C.byref(one), C.byref(one), 0) == INV
    assert paint(None, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), C.byref(one), C.byref(one), 0) == INV
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, C.byref(one), C.byref(one), 0) == INV
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.PMCTL_SPAN_NOTE_ON] = abi.ScriptSpanParam(sp[abi.PMCTL_SPAN_FREQ].f, None)                  # `f` on a u-only field
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), C.byref(one), C.byref(one), 0) == INV
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.PMCTL_SPAN_FREQ] = abi.ScriptSpanParam(None, sp[abi.PMCTL_SPAN_NOTE_ON].u)                  # `u` on an f-only field
    assert controlled(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), C.byref(m._control(rc)), C.byref(m._control(mc_)), 0) == INV
    # controls: NULL, a NULL table, a NULL table array, a NULL value / note_on array, arrays of the wrong kind
    r_ok, m_ok = m._control(rc), m._control(mc_)
    call = lambda r, mm: controlled(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(ctb), r, mm, 0)
    assert call(None, C.byref(m_ok)) == INV and call(C.byref(r_ok), None) == INV
    no_table = m._control(rc); no_table.table = None
    assert call(C.byref(no_table), C.byref(m_ok)) == INV
    broken = abi.ScriptSpanTable.from_buffer_copy(r_ok.table.contents); broken.end = None
    no_array = m._control(rc); no_array.table = C.pointer(broken)
    assert call(C.byref(no_array), C.byref(m_ok)) == INV
    no_value = m._control(mc_); no_value.value = abi.ScriptSpanParam(None, None)
    assert call(C.byref(r_ok), C.byref(no_value)) == INV
    no_on = m._control(mc_); no_on.note_on = abi.ScriptSpanParam(None, None)
    assert call(C.byref(r_ok), C.byref(no_on)) == INV
    wrong = m._control(rc); wrong.value = abi.ScriptSpanParam(r_ok.value.f, r_ok.note_on.u)             # a value with `u`
    assert call(C.byref(wrong), C.byref(m_ok)) == INV
    wrong = m._control(rc); wrong.note_on = abi.ScriptSpanParam(r_ok.value.f, r_ok.note_on.u)           # a note_on with `f`
    assert call(C.byref(wrong), C.byref(m_ok)) == INV
    wrong = m._control(rc); wrong.value, wrong.note_on = r_ok.note_on, r_ok.value                       # the two swapped
    assert call(C.byref(wrong), C.byref(m_ok)) == INV
    patch = abi.PMCtlPatch()
    assert ctx.lib.zh_pmctl_patch_default(C.byref(patch)) == 0 and ctx.lib.zh_pmctl_patch_default(None) == INV
    assert (patch.ctl_curve, [round(x, 6) for x in (patch.ctl_glide, patch.attack, patch.decay, patch.release, patch.sustain_volume)]) == \
        (abi.CURVE_LINEAR, [0.1, 0.025, 0.1, 1.0, 0.5])
    assert (abi.PMCTL_SPAN_FREQ, abi.PMCTL_SPAN_NOTE_ON, abi.PMCTL_SPAN_FIELDS) == (0, 1, 2)
    ctx.sync()                                                         # every refused call left the output and the state alone
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and m.state().tobytes() == state
    assert call(C.byref(r_ok), C.byref(m_ok)) == abi.ZH_OK             # ... and the good call is good
    ctx.sync()
    assert not torch.equal(out.view(torch.int32), before.view(torch.int32)) and m.state().tobytes() != state
    m.close()


def test_capture_and_replay_equal_the_direct_launches():
    """paint_controlled allocates nothing and never synchronises: two buffers recorded into one graph and replayed == the same two
    launched directly, outputs, carried temps and states; a single-stream capture"""
    import torch
    import zang_amd
    from zang_amd import modules as mod, zang
    V, span = 130, mc.SPANS[96]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        ms = [mod.PMCtl(V, c2) for _ in range(2)]
        stales = [util.to_image(np.zeros((V, mc.ROWS), f32)) for _ in range(2)]
        outs = [[util.to_image(mc.base_image(V, 60 + b)) for b in range(2)] for _ in range(2)]
        tables = []
        for b in range(2):
            tbs = mc.streams(V, 96, 700 + b)
            tables.append((_notes(ms[0], tbs[0]), _ctl(ms[0], tbs[1], 4.0), _ctl(ms[0], tbs[2], 2.0)))
        params = ms[0].Params(mc.SR, relative=True, patch=_patch(ms[0]))

        def run(i):
            for b in range(2):
                ms[i].paint_controlled(zang.Span(*span), [outs[i][b]], [None, stales[i], None], params, *tables[b], zero_first=b == 1)
        run(0)                                        # direct; the tables are uploaded here, before the capture records
        c2.sync()
        g = c2.capture(lambda: run(1))
        assert g.kernels() == [("k_pmctl_controlled", 2)], g.kernels()
        g.launch()
        c2.sync()
        for b in range(2):
            assert hc.same_f32(util.from_image(outs[0][b]), util.from_image(outs[1][b])), b
            assert not hc.same_f32(util.from_image(outs[0][b]), mc.base_image(V, 60 + b))
        assert hc.same_f32(util.from_image(stales[0]), util.from_image(stales[1]))
        assert ms[0].state().tobytes() == ms[1].state().tobytes() != bytes(ms[0].state().nbytes)
        g.close()
        for m in ms:
            m.close()
        c2.close()
