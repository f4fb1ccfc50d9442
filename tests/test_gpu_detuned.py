"""GPU: the detuned voice -- zh_detuned_paint (k_detuned) and zh_detuned_paint_spans (k_detuned_spans) -- against
tests/detuned_reference.py: OuterInstrument.paint as the literal sequence of oracle calls, per voice and per sub-span.
Everything on bits: the uint32 views of both output images and of the state's 18 words; any NaN equals any NaN (by position)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import detuned_cases as dc
from tests import detuned_reference as dr
from tests import hostile_cases as hc
from tests import util

pytestmark = pytest.mark.gpu


def _voices(oracle, V):
    return [dr.Voice(oracle, dc.FIRST_SEED + v) for v in range(V)]


def _table(m, tb, names=dr.FIELDS):
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], dc.span_values(tb, names) if names else None)


def _same(got, ref, what):
    assert hc.same_f32(got, ref), (what, hc.first_difference(got, ref))


def _check(m, out, sync, ref, rsync, voices, what):
    _same(util.from_image(out), ref, what)
    if sync is not None:
        _same(util.from_image(sync), rsync, what + " sync")
    gs, rs = dr.struct_state(m.state()), dr.state_words(voices)
    assert dr.same_words(gs, rs), (what + " state", np.argwhere(gs != rs)[:4])


def _params(m, patch, sr=dc.SR, freq=1.0, note_on=False, mode=3):
    return m.Params(sr, freq, note_on, mode, dc.gpu_patch(patch))


@pytest.mark.parametrize("V", [1, 64, 65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_equals_the_reference_per_sub_span(ctx, oracle, V, zero_first):
    """Two consecutive buffers with carried envelope, filter, oscillator and noise state, all three fields from span arrays, both
    outputs: empty sub-spans, one out of order, note-offs, a voice with no sub-span; rows outside [3, 250) keep their bits and
    -0.0 planted in the bases survives exactly where the reference leaves it."""
    from zang_amd import modules as mod, zang
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    voices = _voices(oracle, V)
    for b in range(2):
        tb = dc.tables(V, 1000 * V + b, note_on_first=b == 0)
        base, sbase = dc.base_image(V, 77 + V + b), dc.base_image(V, 177 + V + b)
        ref, rsync = base.copy(), sbase.copy()
        dr.paint_spans(oracle, voices, tb, ref, rsync, dc.SPAN, dc.SR, zero_first, dc.TEST_PATCH)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*dc.SPAN), [out, sync], None, _params(m, dc.TEST_PATCH), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_detuned_spans"], ctx.last_form()
        _check(m, out, sync, ref, rsync, voices, f"V={V} buffer {b}")
        if V > 1:
            assert not dc.same_bits(ref, base) and not dc.same_bits(rsync, sbase)
    m.close()


@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_without_the_sync_output(ctx, oracle, zero_first):
    """outputs[1] NULL: the voice and the state are what they are with it, over two buffers; given as None and left out"""
    from zang_amd import modules as mod, zang
    V = 65
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    voices = _voices(oracle, V)
    for b in range(2):
        tb = dc.tables(V, 500 + b, note_on_first=b == 0)
        base = dc.base_image(V, 60 + b)
        ref = base.copy()
        dr.paint_spans(oracle, voices, tb, ref, None, dc.SPAN, dc.SR, zero_first, dc.TEST_PATCH)
        out = util.to_image(base)
        m.paint_spans(zang.Span(*dc.SPAN), [out, None] if b else [out], None, _params(m, dc.TEST_PATCH), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        _check(m, out, None, ref, None, voices, f"buffer {b}")
    m.close()


@pytest.mark.parametrize("how", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, how):
    """broadcast: no span arrays at all (span_params NULL), one value of every field for every voice.  per_voice: all three from
    per-voice device arrays.  mixed: freq per sub-span, note_on and mode per voice."""
    import torch
    from zang_amd import modules as mod, zang
    V = 65
    tb = dc.tables(V, 4242)
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    voices = _voices(oracle, V)
    rng = np.random.default_rng(5)
    if how == "broadcast":
        dflt = {"freq": np.float32(330.0), "note_on": 1, "mode": 1}
        params = _params(m, dc.TEST_PATCH, freq=330.0, note_on=True, mode=1)
        names = ()
    else:
        dflt = {"freq": rng.uniform(110.0, 880.0, V).astype(np.float32), "note_on": (np.arange(V) % 3 != 0).astype(np.uint32),
                "mode": (np.arange(V) % 4).astype(np.uint32)}
        params = _params(m, dc.TEST_PATCH, freq=util.dev(dflt["freq"]), note_on=util.dev(dflt["note_on"].astype(np.uint8)),
                         mode=torch.from_numpy(dflt["mode"].astype(np.int32)).cuda())
        names = () if how == "per_voice" else ("freq",)
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base, sbase = dc.base_image(V, 3), dc.base_image(V, 4)
    ref, rsync = base.copy(), sbase.copy()
    dr.paint_spans(oracle, voices, lean, ref, rsync, dc.SPAN, dc.SR, False, dc.TEST_PATCH, dflt=dflt)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*dc.SPAN), [out, sync], None, params, _table(m, tb, names))
    ctx.sync()
    _check(m, out, sync, ref, rsync, voices, how)
    assert not dc.same_bits(ref, base)
    m.close()


@pytest.mark.parametrize("V", [1, 65])
def test_uniform_paint_equals_the_span_form_with_one_full_sub_span(ctx, oracle, V, monkeypatch):
    """zh_detuned_paint: V voices, each with its own freq, note_on, mode and note_id_changed, painting the span twice (ADD, then
    ZERO_FIRST) with carried state == the reference == zh_detuned_paint_spans over one full sub-span per voice == the same paint
    through the walk (dispatch row detuned_uniform_walk)"""
    import torch
    from zang_amd import modules as mod, zang
    S, E = dc.SPAN
    ms = [mod.Detuned(V, ctx, dc.FIRST_SEED) for _ in range(3)]
    voices = _voices(oracle, V)
    for b in range(2):
        tb = dc.one_span_tables(V, 77 * V + b)
        base, sbase = dc.base_image(V, 31 + V + b), dc.base_image(V, 131 + V + b)
        ref, rsync = base.copy(), sbase.copy()
        dr.paint_spans(oracle, voices, tb, ref, rsync, dc.SPAN, dc.SR, b == 1, dc.TEST_PATCH)
        params = _params(ms[0], dc.TEST_PATCH, freq=util.dev(tb["freq"][0]), note_on=util.dev(tb["note_on"][0].astype(np.uint8)),
                         mode=torch.from_numpy(tb["mode"][0].astype(np.int32)).cuda())
        outs = [(util.to_image(base), util.to_image(sbase)) for _ in range(3)]
        ms[0].paint(zang.Span(S, E), list(outs[0]), [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_detuned"], ctx.last_form()
        ms[1].paint_spans(zang.Span(S, E), list(outs[1]), None, _params(ms[1], dc.TEST_PATCH), _table(ms[1], tb), zero_first=b == 1)
        util.set_form(monkeypatch, detuned_uniform_walk=1)
        ms[2].paint(zang.Span(S, E), list(outs[2]), [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_detuned_spans"], ctx.last_form()
        util.del_form(monkeypatch, "detuned_uniform_walk")
        for i, what in enumerate(("uniform", "one sub-span", "uniform through the walk")):
            _check(ms[i], outs[i][0], outs[i][1], ref, rsync, voices, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


def test_the_default_patch_over_ten_buffers(ctx, oracle):
    """the reference's constants over ten buffers of 256 frames at 65 voices, each with its own freq and mode: attack, decay, a
    note-off in the seventh, release; the frequency image in the odd buffers only"""
    import torch
    from zang_amd import modules as mod, zang
    V, F = 65, 256
    rng = np.random.default_rng(11)
    freq = rng.uniform(110.0, 880.0, V).astype(np.float32)
    mode = (np.arange(V) % 4).astype(np.uint32)
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    voices = _voices(oracle, V)
    temps = [np.zeros(F, np.float32) for _ in range(4)]
    loud = 0.0
    for b in range(10):
        ref, rsync = np.zeros((V, F), np.float32), (np.zeros((V, F), np.float32) if b % 2 else None)
        for v in range(V):
            dr.outer_paint(oracle, voices[v], 0, F, (ref[v], None if rsync is None else rsync[v]), temps, b == 0, dc.SR, freq[v], b < 6,
                           int(mode[v]), dc.DEFAULT_PATCH)
        out = ctx.image(F, V, fill=0.0)
        sync = ctx.image(F, V, fill=0.0) if b % 2 else None
        m.paint(zang.Span(0, F), [out, sync], [], b == 0, m.Params(dc.SR, util.dev(freq), b < 6, torch.from_numpy(mode.astype(np.int32)).cuda()))
        ctx.sync()
        _check(m, out, sync, ref, rsync, voices, f"buffer {b}")
        loud = max(loud, float(np.abs(ref).max()))
    assert loud > 0.1 and all(int(v.env.state) == oracle.ENV_RELEASE for v in voices)
    m.close()


def test_planted_warble_reaches_every_arm_of_pow(ctx, oracle):
    """noise_filter.l planted through set_state in 22 of 130 voices (dc.PLANTED, each in mode 0 and mode 1): the integer loop, the
    reciprocal arm, denormal results, underflow to 0, overflow to inf and the NaN that follows; two buffers"""
    from zang_amd import modules as mod, zang
    V = 130
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    st = m.state()
    voices = _voices(oracle, V)
    planted = dc.PLANTED + dc.PLANTED
    at = [3 * i + 5 for i in range(len(planted))]                        # among ordinary voices, in both waves and the tail
    tbs = [dc.tables(V, 2200 + b, note_on_first=b == 0) for b in range(2)]
    for i, (v, w) in enumerate(zip(at, planted)):
        st["noise_filter"]["l"][v] = w
        voices[v].noise_filter.l = float(np.float32(w))
        for tb in tbs:
            tb["mode"][:, v] = i // len(dc.PLANTED)
            tb["count"][v], tb["start"][0, v], tb["end"][0, v] = 1, dc.SPAN[0] + i, dc.SPAN[1] - i
    m.set_state(st)
    seen_nan = seen_inf = seen_denormal = False
    for b, tb in enumerate(tbs):
        base, sbase = dc.base_image(V, 40 + b), dc.base_image(V, 50 + b)
        ref, rsync = base.copy(), sbase.copy()
        dr.paint_spans(oracle, voices, tb, ref, rsync, dc.SPAN, dc.SR, True, dc.TEST_PATCH)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*dc.SPAN), [out, sync], None, _params(m, dc.TEST_PATCH), _table(m, tb), zero_first=True)
        ctx.sync()
        _check(m, out, sync, ref, rsync, voices, f"buffer {b}")
        seen_nan |= bool(np.isnan(ref).any()); seen_inf |= bool(np.isinf(rsync).any())
        seen_denormal |= bool(((np.abs(rsync) > 0) & (np.abs(rsync) < 1.17e-38)).any())
        assert dc.nan_share(ref[:, 3:250], rsync[:, 3:250]) <= dc.NAN_CAP
    assert seen_nan and seen_inf and seen_denormal
    m.close()


@functools.lru_cache(maxsize=None)
def _hostile_freq_tables():
    """Every value of dc.HOSTILE_FREQ in the middle sub-span (100 frames) of a voice whose other two are ordinary: hostile voice i
    once alone in its wave (voice 64 * i) and once among the other hostile ones (voices 64 * n ...); everything else ordinary."""
    n = len(dc.HOSTILE_FREQ)
    V = 64 * n + 64
    tb = dc.tables(V, 31337)
    for i, x in enumerate(dc.HOSTILE_FREQ):
        for v in (64 * i, 64 * n + i):
            tb["count"][v] = 3
            tb["start"][:3, v], tb["end"][:3, v] = (3, 80, 180), (80, 180, 250)
            tb["freq"][:3, v] = (220.0, x, 440.0)
            tb["note_on"][:3, v] = 1
    return V, tb


def test_hostile_freq_in_one_sub_span(ctx, oracle):
    from zang_amd import modules as mod, zang
    V, tb = _hostile_freq_tables()
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    voices = _voices(oracle, V)
    base, sbase = dc.base_image(V, 90), dc.base_image(V, 91)
    ref, rsync = base.copy(), sbase.copy()
    dr.paint_spans(oracle, voices, tb, ref, rsync, dc.SPAN, dc.SR, False, dc.TEST_PATCH)
    share = dc.nan_share(ref[:, 3:250], rsync[:, 3:250])
    print("hostile freq: NaN share", share)
    assert 0.0 < share <= dc.NAN_CAP
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*dc.SPAN), [out, sync], None, _params(m, dc.TEST_PATCH), _table(m, tb))
    ctx.sync()
    _check(m, out, sync, ref, rsync, voices, "hostile freq")
    m.close()


def _uniform_run(ctx, oracle, V, sample_rate, patch, what):
    """two uniform paints with carried state (note_id_changed, then a note-off), per-voice freq and mode, both outputs"""
    import torch
    from zang_amd import modules as mod, zang
    S, E = dc.SPAN
    rng = np.random.default_rng(17)
    freq = rng.uniform(110.0, 880.0, V).astype(np.float32)
    mode = (np.arange(V) % 2).astype(np.uint32)
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    voices = _voices(oracle, V)
    temps = [np.zeros(dc.ROWS, np.float32) for _ in range(4)]
    shares = []
    for b in range(2):
        base, sbase = dc.base_image(V, 900 + b), dc.base_image(V, 910 + b)
        ref, rsync = base.copy(), sbase.copy()
        for v in range(V):
            dr.outer_paint(oracle, voices[v], S, E, (ref[v], rsync[v]), temps, b == 0, sample_rate, freq[v], b == 0, int(mode[v]), patch)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint(zang.Span(S, E), [out, sync], [], b == 0,
                _params(m, patch, sr=sample_rate, freq=util.dev(freq), note_on=b == 0, mode=torch.from_numpy(mode.astype(np.int32)).cuda()))
        ctx.sync()
        _check(m, out, sync, ref, rsync, voices, f"{what} paint {b}")
        shares.append(dc.nan_share(ref[:, S:E], rsync[:, S:E]))
    print(what, "NaN shares", shares)
    m.close()


def _hostile_sr_reference(oracle, V, sample_rate):
    """three span paints of V voices with carried state -- an ordinary sample rate, the hostile one, the ordinary one again (a
    state the hostile paint left NaN stays NaN) -- on whole images: -> [(table, base, sync base, ref, sync ref, rate)], the
    voices, the NaN share of everything compared"""
    voices = _voices(oracle, V)
    runs = []
    for b, sr in enumerate((dc.SR, sample_rate, dc.SR)):
        tb = dc.tables(V, 700 + b, note_on_first=b == 0)
        base, sbase = dc.base_image(V, 900 + b), dc.base_image(V, 910 + b)
        ref, rsync = base.copy(), sbase.copy()
        dr.paint_spans(oracle, voices, tb, ref, rsync, dc.SPAN, sr, False, dc.TEST_PATCH)
        runs.append((tb, base, sbase, ref, rsync, sr))
    return runs, voices, dc.nan_share(*[r[3] for r in runs], *[r[4] for r in runs])


@pytest.mark.parametrize("sample_rate", dc.HOSTILE_SR, ids=["zero", "negative", "nan", "inf", "denormal"])
def test_hostile_sample_rates_equal_the_reference(ctx, oracle, sample_rate):
    """the sample rate is uniform over a call, so a hostile one reaches every voice of its paint: it sits between two ordinary
    paints of the same 65 voices, and whole images are compared.  The oracle alone: NaN shares 0.10 (0, NaN, 1e-40) and 0 (-48000, inf)."""
    from zang_amd import modules as mod, zang
    V = 65
    runs, voices, share = _hostile_sr_reference(oracle, V, sample_rate)
    print("sample_rate", sample_rate, "NaN share", share)
    assert share <= dc.NAN_CAP
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    for b, (tb, base, sbase, ref, rsync, sr) in enumerate(runs):
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*dc.SPAN), [out, sync], None, _params(m, dc.TEST_PATCH, sr=sr), _table(m, tb))
        ctx.sync()
        _same(util.from_image(out), ref, f"sample_rate {sample_rate} paint {b}")
        _same(util.from_image(sync), rsync, f"sample_rate {sample_rate} paint {b} sync")
    gs, rs = dr.struct_state(m.state()), dr.state_words(voices)
    assert dr.same_words(gs, rs), np.argwhere(gs != rs)[:4]
    m.close()


@pytest.mark.parametrize("field,value", [("res", 1.5), ("cutoff_hz", -1.0), ("attack", 0.0), ("volume", float("nan"))])
def test_hostile_patch_values_equal_the_reference(ctx, oracle, field, value):
    import dataclasses
    _uniform_run(ctx, oracle, 5, dc.SR, dataclasses.replace(dc.TEST_PATCH, **{field: value}), f"{field} {value}")


def test_state_round_trip(ctx, oracle):
    """get_state after set_state gives the words back (the taps, which the voice does not hold, as zeros); a paint from the set
    state is the reference's from the same state"""
    from zang_amd import modules as mod, zang
    V = 3
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    st = m.state()
    fresh = _voices(oracle, V)
    assert np.array_equal(dr.struct_state(st), dr.state_words(fresh))                # create == init(), seeds included
    rng = np.random.default_rng(2)
    st["noise"]["r"][:] = rng.integers(1, 2 ** 63, (V, 4), dtype=np.uint64)
    for obj, field, kind in dr.STATE[1:]:
        st[obj][field][:] = rng.uniform(-0.5, 0.5, V).astype(np.float32) if kind == "f" else rng.integers(0, 5, V)
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    for v in range(V):
        fresh[v].load(st, v)
    S, E = dc.SPAN
    base = dc.base_image(V, 8)
    ref = base.copy()
    temps = [np.zeros(dc.ROWS, np.float32) for _ in range(4)]
    for v in range(V):
        dr.outer_paint(oracle, fresh[v], S, E, (ref[v], None), temps, False, dc.SR, 220.0, True, 0, dc.TEST_PATCH)
    out = util.to_image(base)
    m.paint(zang.Span(S, E), [out], [], False, _params(m, dc.TEST_PATCH, freq=220.0, note_on=True, mode=0))
    ctx.sync()
    _check(m, out, None, ref, None, fresh, "from a set state")
    m.close()


def test_paints_span_paints_and_a_graph_replay_mix(oracle):
    """a span paint, a captured span paint replayed twice and a uniform paint of ONE zh_detuned == the same four paints made
    directly on another (both images and the state); a single-stream capture"""
    import torch
    import zang_amd
    from zang_amd import modules as mod, zang
    V = 65
    tb = dc.tables(V, 5150)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        me, mg = mod.Detuned(V, c2, dc.FIRST_SEED), mod.Detuned(V, c2, dc.FIRST_SEED)
        base, sbase = dc.base_image(V, 8), dc.base_image(V, 9)
        out_e, out_g, sync_e, sync_g = util.to_image(base), util.to_image(base), util.to_image(sbase), util.to_image(sbase)
        tab_e, tab_g = _table(me, tb), _table(mg, tb)
        tab_g.device(c2.device, list(dr.FIELDS))      # uploaded before the capture records
        span = zang.Span(*dc.SPAN)
        spans = lambda m, out, sync, tab: m.paint_spans(span, [out, sync], None, _params(m, dc.TEST_PATCH), tab)
        plain = lambda m, out, sync: m.paint(span, [out, sync], [], False, _params(m, dc.TEST_PATCH, freq=330.0, note_on=False, mode=1))
        for _ in range(3):
            spans(me, out_e, sync_e, tab_e)
        plain(me, out_e, sync_e)
        c2.sync()
        spans(mg, out_g, sync_g, tab_g)
        g = c2.capture(lambda: spans(mg, out_g, sync_g, tab_g))
        g.launch(); g.launch()
        plain(mg, out_g, sync_g)
        c2.sync()
        assert torch.equal(out_e.view(torch.int32), out_g.view(torch.int32)) and torch.equal(sync_e.view(torch.int32), sync_g.view(torch.int32))
        assert me.state().tobytes() == mg.state().tobytes()
        assert not torch.equal(out_e, util.to_image(base))
        g.close(); me.close(); mg.close()
        c2.close()


def test_refusals(ctx):
    import torch
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf
    V = 8
    tb = dc.tables(V, 1)
    m = mod.Detuned(V, ctx, dc.FIRST_SEED)
    out, sync = ctx.image(dc.ROWS, V, fill=0.25), ctx.image(dc.ROWS, V, fill=0.5)
    before, sbefore = out.clone(), sync.clone()
    state = m.state().tobytes()
    span = zang.Span(*dc.SPAN)
    good = _params(m, dc.TEST_PATCH)
    assert m._paint_spans(span, [out, sync], None, good, _table(m, tb), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_spans(span, [out[:50], sync], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID      # too few rows
    assert m._paint_spans(span, [out[:, :V - 1], sync], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID  # too few voices
    assert m._paint_spans(span, [out, sync[:50]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID      # the second output too small
    wide, marker = ctx.image(dc.ROWS, 2 * V, fill=0.5), ctx.last_form()    # outputs[1] shares a float with outputs[0]: refused, no launch
    assert m._paint_spans(span, [out, out], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID                  # the same image
    assert m._paint_spans(span, [wide[:, :V], wide[:, V - 1:2 * V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID   # one column in common
    assert ctx.last_form() == marker
    with pytest.raises(abi.ZangHipError):
        m.paint(span, [out[:50]], [], False, good)
    outs = (abi.Buf * 2)(as_buf(out), as_buf(sync))
    null0 = (abi.Buf * 2)(abi.Buf(), as_buf(sync))
    ctb, sp = _table(m, tb).device(ctx.device, list(dr.FIELDS))
    cp = m._cparams(good)
    assert ctx.lib.zh_detuned_paint(m.handle, span.start, span.end, null0, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # outputs[0] NULL
    assert ctx.lib.zh_detuned_paint_spans(m.handle, span.start, span.end, null0, None, C.byref(cp), sp, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_detuned_paint(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert ctx.lib.zh_detuned_paint(m.handle, span.end, span.start, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # end < start
    assert ctx.lib.zh_detuned_paint(m.handle, span.start, span.end, None, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID   # no images
    assert ctx.lib.zh_detuned_paint(m.handle, span.start, span.end, outs, None, abi.Bool(), None, 0) == abi.ZH_ERR_INVALID          # no params
    assert ctx.lib.zh_detuned_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, None, 0) == abi.ZH_ERR_INVALID  # no table
    bad = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
    bad[abi.DETUNED_SPAN_MODE] = abi.ScriptSpanParam(sp[abi.DETUNED_SPAN_FREQ].f, None)   # `f` on a u-only field
    assert ctx.lib.zh_detuned_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    empty = abi.ScriptSpanTable(0, 0, ctb.count, ctb.start, ctb.end, ctb.note_id_changed)   # max_spans == 0
    assert ctx.lib.zh_detuned_paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(empty), 0) == abi.ZH_ERR_INVALID
    ctx.sync()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and torch.equal(sync.view(torch.int32), sbefore.view(torch.int32))
    assert m.state().tobytes() == state                                                   # nothing painted
    m.close()
