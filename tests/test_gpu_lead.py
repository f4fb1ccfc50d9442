"""GPU: the two monophonic leads -- zh_porta_paint[_spans] and zh_vibrato_paint[_spans] (k_lead_spans) -- against
tests/lead_reference.py: Instrument.paint of examples/example_portamento.zig and examples/example_vibrato.zig as the literal
sequence of oracle calls, per voice and per sub-span, prev_note_on carried in Python.  Everything on bits: the uint32 views of both
output images and of every state word; any NaN equals any NaN (by position)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import lead_cases as lc
from tests import lead_reference as lr
from tests import util

pytestmark = pytest.mark.gpu
both = pytest.mark.parametrize("kind", lc.KINDS, ids=lc.KIND_IDS)


def _table(m, tb, names=lr.FIELDS):
    return m.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], lc.span_values(tb, names) if names else None)


def _same(got, ref, what):
    assert hc.same_f32(got, ref), (what, hc.first_difference(got, ref))


def _check(kind, m, out, sync, ref, rsync, voices, what):
    _same(util.from_image(out), ref, what)
    if sync is not None:
        _same(util.from_image(sync), rsync, what + " sync")
    gs, rs = lr.struct_state(kind.voice, m.state()), lr.state_words(voices)
    assert lr.same_words(kind.voice, gs, rs), (what + " state", np.argwhere(gs != rs)[:4])


def _params(kind, m, patch, sr=lc.SR, freq=1.0, note_on=False):
    return m.Params(sr, freq, note_on, kind.gpu_patch(patch))


def _uniform_ref(oracle, kind, voices, S, E, ref, rsync, nic, sr, freq, note_on, patch):
    """Instrument.paint over [S, E) for every voice; nic, freq and note_on scalars or per-voice arrays"""
    temps = [np.zeros(lc.ROWS, np.float32) for _ in range(3)]
    at = lambda x, v: x[v] if isinstance(x, np.ndarray) else x
    for v in range(len(voices)):
        kind.paint(oracle, voices[v], S, E, (ref[v], None if rsync is None else rsync[v]), temps, at(nic, v), sr, at(freq, v), bool(at(note_on, v)), patch)


@both
@pytest.mark.parametrize("V", [1, 64, 65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_equals_the_reference_per_sub_span(ctx, oracle, kind, V, zero_first):
    """Two consecutive buffers with carried state (prev_note_on among it), both fields from span arrays, both outputs: empty
    sub-spans, one out of order, note-offs, a voice with no sub-span; rows outside [3, 250) keep their bits and -0.0 planted in
    the bases survives exactly where the reference leaves it.  The sub-spans reached hold all four (prev_note_on, note_on) pairs
    and on->on with note_id_changed set and clear."""
    from zang_amd import zang
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    tbs = [lc.tables(V, 1000 * V + b, note_on_first=b == 0) for b in range(2)]
    assert lc.covers_every_pair(tbs), lc.pairs(tbs)
    for b, tb in enumerate(tbs):
        base, sbase = lc.base_image(V, 77 + V + b), lc.base_image(V, 177 + V + b)
        ref, rsync = base.copy(), sbase.copy()
        lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, zero_first, kind.test_patch)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, _params(kind, m, kind.test_patch), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_lead_spans"], ctx.last_form()
        _check(kind, m, out, sync, ref, rsync, voices, f"V={V} buffer {b}")
        assert not lc.same_bits(ref, base) and not lc.same_bits(rsync, sbase)
    m.close()


@both
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_without_the_sync_output(ctx, oracle, kind, zero_first):
    """outputs[1] NULL: the voice and the state are what they are with it, over two buffers; given as None and left out"""
    from zang_amd import zang
    V = 65
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    for b in range(2):
        tb = lc.tables(V, 500 + b, note_on_first=b == 0)
        base = lc.base_image(V, 60 + b)
        ref = base.copy()
        lr.paint_spans(oracle, kind.paint, voices, tb, ref, None, lc.SPAN, lc.SR, zero_first, kind.test_patch)
        out = util.to_image(base)
        m.paint_spans(zang.Span(*lc.SPAN), [out, None] if b else [out], None, _params(kind, m, kind.test_patch), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        _check(kind, m, out, None, ref, None, voices, f"buffer {b}")
    m.close()


@both
@pytest.mark.parametrize("how", ["broadcast", "per_voice", "mixed"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, kind, how):
    """broadcast: no span arrays at all (span_params NULL), one value of both fields for every voice.  per_voice: both from
    per-voice device arrays.  mixed: freq per sub-span, note_on per voice."""
    from zang_amd import zang
    V = 65
    tb = lc.tables(V, 4242)
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    rng = np.random.default_rng(5)
    if how == "broadcast":
        dflt = {"freq": np.float32(330.0), "note_on": 1}
        params = _params(kind, m, kind.test_patch, freq=330.0, note_on=True)
        names = ()
    else:
        dflt = {"freq": rng.uniform(110.0, 880.0, V).astype(np.float32), "note_on": (np.arange(V) % 3 != 0).astype(np.uint32)}
        params = _params(kind, m, kind.test_patch, freq=util.dev(dflt["freq"]), note_on=util.dev(dflt["note_on"].astype(np.uint8)))
        names = () if how == "per_voice" else ("freq",)
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base, sbase = lc.base_image(V, 3), lc.base_image(V, 4)
    ref, rsync = base.copy(), sbase.copy()
    lr.paint_spans(oracle, kind.paint, voices, lean, ref, rsync, lc.SPAN, lc.SR, False, kind.test_patch, dflt=dflt)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, params, _table(m, tb, names))
    ctx.sync()
    _check(kind, m, out, sync, ref, rsync, voices, how)
    assert not lc.same_bits(ref, base)
    m.close()


@both
@pytest.mark.parametrize("V", [1, 65])
def test_plain_paint_equals_the_span_form_with_one_full_sub_span(ctx, oracle, kind, V):
    """zh_X_paint: V voices, each with its own freq, note_on and note_id_changed, painting the span three times (ADD, ZERO_FIRST,
    ADD) with carried state == the reference == zh_X_paint_spans over one full sub-span per voice"""
    from zang_amd import zang
    S, E = lc.SPAN
    ms = [kind.module()(V, ctx) for _ in range(2)]
    voices = kind.voices(oracle, V)
    for b in range(3):
        tb = lc.one_span_tables(V, 77 * V + b)
        base, sbase = lc.base_image(V, 31 + V + b), lc.base_image(V, 131 + V + b)
        ref, rsync = base.copy(), sbase.copy()
        lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, b == 1, kind.test_patch)
        params = _params(kind, ms[0], kind.test_patch, freq=util.dev(tb["freq"][0]), note_on=util.dev(tb["note_on"][0].astype(np.uint8)))
        outs = [(util.to_image(base), util.to_image(sbase)) for _ in range(2)]
        ms[0].paint(zang.Span(S, E), list(outs[0]), [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ms[1].paint_spans(zang.Span(S, E), list(outs[1]), None, _params(kind, ms[1], kind.test_patch), _table(ms[1], tb), zero_first=b == 1)
        ctx.sync()
        for i, what in enumerate(("plain", "one sub-span")):
            _check(kind, ms[i], outs[i][0], outs[i][1], ref, rsync, voices, f"V={V} paint {b} {what}")
    for m in ms:
        m.close()


# ten buffers: (note_id_changed, frequency factor, note_on).  The glide of 0.5 s begun in buffer 2 and the release of 1 s begun in
# buffer 5 span buffers; buffer 7 is on after off (the envelope restarts, the glide is instantaneous), buffer 8 a new note while on
TEN = [(True, 1.0, True), (False, 1.0, True), (True, 1.5, True), (False, 1.5, True), (False, 1.5, True), (False, 1.5, False),
       (False, 1.5, False), (True, 0.75, True), (True, 2.0, True), (False, 2.0, False)]


@both
def test_the_default_patch_over_ten_buffers(ctx, oracle, kind):
    """the reference's constants over ten buffers of 256 frames at 65 voices, each with its own freq; prev_note_on and the state
    carry across them; the frequency image in the odd buffers only"""
    from zang_amd import zang
    V, F = 65, 256
    rng = np.random.default_rng(11)
    freq = rng.uniform(110.0, 880.0, V).astype(np.float32)
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    loud, moved = 0.0, False
    for b, (nic, mul, on) in enumerate(TEN):
        fb = (freq * np.float32(mul)).astype(np.float32)
        ref, rsync = np.zeros((V, F), np.float32), (np.zeros((V, F), np.float32) if b % 2 else None)
        _uniform_ref(oracle, kind, voices, 0, F, ref, rsync, nic, lc.SR, fb, on, kind.default_patch)
        out = ctx.image(F, V, fill=0.0)
        sync = ctx.image(F, V, fill=0.0) if b % 2 else None
        m.paint(zang.Span(0, F), [out, sync], [], nic, m.Params(lc.SR, util.dev(fb), on))
        ctx.sync()
        _check(kind, m, out, sync, ref, rsync, voices, f"buffer {b}")
        loud = max(loud, float(np.abs(ref).max()))
        if b == 3:                                                   # the frequency image moves inside the buffer: glide, or vibrato
            moved = bool((rsync[:, 0] != rsync[:, -1]).all())
            if kind is lc.PORTA:                                     # the glide begun in buffer 2 is unfinished and prev_note_on is set
                assert all(0.0 < float(v.porta.painter.t) < 1.0 and v.prev_note_on for v in voices)
    assert loud > 0.1 and moved
    if kind is lc.PORTA:
        assert all(int(v.env.state) == oracle.ENV_RELEASE and not v.prev_note_on for v in voices)
    m.close()


@pytest.mark.parametrize("tag", [0, 1, 2, 3], ids=["instantaneous", "linear", "squared", "cubed"])
def test_porta_every_glide_curve(ctx, oracle, tag):
    from zang_amd import zang
    kind, V = lc.PORTA, 65
    patch = dataclasses.replace(kind.test_patch, glide_curve=tag, glide=lc.ms(90))
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    for b in range(2):
        tb = lc.tables(V, 900 + b, note_on_first=b == 0)
        base, sbase = lc.base_image(V, 20 + b), lc.base_image(V, 30 + b)
        ref, rsync = base.copy(), sbase.copy()
        lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, False, patch)
        out, sync = util.to_image(base), util.to_image(sbase)
        m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, _params(kind, m, patch), _table(m, tb))
        ctx.sync()
        _check(kind, m, out, sync, ref, rsync, voices, f"tag {tag} buffer {b}")
    m.close()


def test_porta_a_note_on_while_prev_note_on_is_set_does_not_restart_the_envelope(ctx, oracle):
    """buffer 0: a note; buffer 1: a NEW note id arrives at frame 40 while the first is still on.  prev_note_on, set by buffer 0,
    keeps the envelope where it is (no second attack: it never falls back toward 0 and never leaves sustain) and makes the glide
    a curve instead of a jump."""
    from zang_amd import zang
    kind, V, F = lc.PORTA, 3, 256
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    ones = lambda x, dt: np.full((1, V), x, dt)
    two = {"count": np.full(V, 2, np.uint32), "start": np.array([[0] * V, [40] * V], np.uint32), "end": np.array([[40] * V, [F] * V], np.uint32),
           "nic": np.array([[0] * V, [1] * V], np.uint8), "freq": np.array([[220.0] * V, [440.0] * V], np.float32), "note_on": np.ones((2, V), np.uint32)}
    one = {"count": np.ones(V, np.uint32), "start": ones(0, np.uint32), "end": ones(F, np.uint32), "nic": ones(1, np.uint8),
           "freq": ones(220.0, np.float32), "note_on": ones(1, np.uint32)}
    for b, tb in enumerate((one, two)):
        ref, rsync = np.zeros((V, F), np.float32), np.zeros((V, F), np.float32)
        lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, (0, F), lc.SR, True, kind.test_patch)
        out, sync = ctx.image(F, V, fill=0.5), ctx.image(F, V, fill=0.5)
        m.paint_spans(zang.Span(0, F), [out, sync], None, _params(kind, m, kind.test_patch), _table(m, tb), zero_first=True)
        ctx.sync()
        _check(kind, m, out, sync, ref, rsync, voices, f"buffer {b}")
    st = m.state()
    assert (st["env"]["state"] == oracle.ENV_SUSTAIN).all() and (st["prev_note_on"] == 1).all()
    got = util.from_image(sync)
    assert 220.0 < got[0, 45] < 440.0 and got[0, 100] == 440.0      # a glide of 30 frames, not a jump
    m.close()


def test_vibrato_a_frequency_out_of_range_paints_nothing_and_the_adds_still_happen(ctx, oracle):
    """per-sub-span freq either side of sample_rate / 8 = 6000 and below 0, over images holding -0.0 (from frame 200 on in the odd
    voices): where the PulseOsc paints nothing out0 += 0 still runs, so -0.0 becomes +0.0 inside the sub-span and stays outside"""
    from zang_amd import zang
    kind, V = lc.VIBRATO, 65
    patch = dataclasses.replace(kind.test_patch, depth=0.01)
    tb = lc.tables(V, 606)
    rng = np.random.default_rng(9)
    tb["freq"][:] = rng.choice(np.array([5900.0, 5999.0, 6000.0, 6001.0, 6100.0, -1.0, -220.0, 440.0], np.float32), tb["freq"].shape)
    tb["note_on"][:] = 1
    tb["count"][1], tb["start"][0, 1], tb["end"][0, 1], tb["freq"][0, 1] = 1, 180, 230, 7000.0     # an odd voice, all -0.0 from 200 on
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    base, sbase = lc.base_image(V, 12), lc.base_image(V, 13)
    ref, rsync = base.copy(), sbase.copy()
    lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, False, patch)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, _params(kind, m, patch), _table(m, tb))
    ctx.sync()
    _check(kind, m, out, sync, ref, rsync, voices, "out of range")
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (bits(ref[1, 200:230]) == 0).all() and (bits(ref[1, 230:250]) == 0x80000000).all() and int(voices[1].osc.cnt) == 0
    m.close()


@both
def test_hostile_freq_in_the_last_sub_span(ctx, oracle, kind):
    from zang_amd import zang
    V, tb = lc.hostile_freq_tables()
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    base, sbase = lc.base_image(V, 90), lc.base_image(V, 91)
    ref, rsync = base.copy(), sbase.copy()
    lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, False, kind.test_patch)
    share = lc.worst_row_nan_share(ref, rsync)
    print(kind.name, "hostile freq: worst NaN share of a voice", share)
    assert 0.0 < share <= lc.NAN_CAP
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint_spans(zang.Span(*lc.SPAN), [out, sync], None, _params(kind, m, kind.test_patch), _table(m, tb))
    ctx.sync()
    _check(kind, m, out, sync, ref, rsync, voices, "hostile freq")
    m.close()


def _call_wide(ctx, oracle, kind, sample_rate, patch, what):
    """a clean plain paint over [3, 200), then one over [200, 250) with the call-wide hostile value; 65 voices with their own freq,
    note_on and note_id_changed in each; both outputs; the cap is asserted, then images and state words are compared"""
    from zang_amd import zang
    V = 65
    S, E = lc.SPAN
    rng = np.random.default_rng(17)
    m = kind.module()(V, ctx)
    voices = kind.voices(oracle, V)
    base, sbase = lc.base_image(V, 900), lc.base_image(V, 910)
    ref, rsync = base.copy(), sbase.copy()
    out, sync = util.to_image(base), util.to_image(sbase)
    for b, (s, e, sr, p) in enumerate(((S, lc.HOSTILE_FROM, lc.SR, kind.test_patch), (lc.HOSTILE_FROM, E, sample_rate, patch))):
        freq = rng.uniform(110.0, 880.0, V).astype(np.float32)
        nic = rng.integers(0, 2, V).astype(np.uint8)
        on = np.ones(V, np.uint8) if b == 0 else (np.arange(V) % 3 != 0).astype(np.uint8)
        _uniform_ref(oracle, kind, voices, s, e, ref, rsync, nic, sr, freq, on, p)
        m.paint(zang.Span(s, e), [out, sync], [], util.dev(nic), _params(kind, m, p, sr=sr, freq=util.dev(freq), note_on=util.dev(on)))
    ctx.sync()
    share = lc.worst_row_nan_share(ref, rsync)
    print(kind.name, what, "worst NaN share of a voice", share)
    assert share <= lc.NAN_CAP
    _check(kind, m, out, sync, ref, rsync, voices, what)
    m.close()


@both
@pytest.mark.parametrize("sample_rate", lc.HOSTILE_SR, ids=["zero", "negative", "nan", "inf", "denormal"])
def test_hostile_sample_rates_equal_the_reference(ctx, oracle, kind, sample_rate):
    _call_wide(ctx, oracle, kind, sample_rate, kind.test_patch, f"sample_rate {sample_rate}")


@pytest.mark.parametrize("kind,field,value", [(lc.PORTA, "glide", 0.0), (lc.PORTA, "glide", float("nan")), (lc.PORTA, "attack", 0.0),
                                              (lc.VIBRATO, "depth", float("nan")), (lc.VIBRATO, "color", 2.0), (lc.VIBRATO, "vib_hz", -1.0)],
                         ids=["glide0", "glide_nan", "attack0", "depth_nan", "color2", "vib_hz_neg"])
def test_hostile_patch_values_equal_the_reference(ctx, oracle, kind, field, value):
    _call_wide(ctx, oracle, kind, lc.SR, dataclasses.replace(kind.test_patch, **{field: value}), f"{field} {value}")


@both
def test_state_round_trip(ctx, oracle, kind):
    """get_state after set_state gives the words back; a paint from the set state is the reference's from the same state.
    Portamento: voice 0 carries prev_note_on = 1 with its envelope mid-release, and the note-on that follows does not restart it."""
    from zang_amd import zang
    V = 3
    m = kind.module()(V, ctx)
    st = m.state()
    fresh = kind.voices(oracle, V)
    assert np.array_equal(lr.struct_state(kind.voice, st), lr.state_words(fresh))        # create == init()
    rng = np.random.default_rng(2)
    for obj, field, k in kind.voice.STATE:
        col = st[field] if obj is None else st[obj][field]
        col[:] = rng.uniform(0.05, 0.5, V).astype(np.float32) if k == "f" else rng.integers(0, 5, V)
    if kind is lc.PORTA:
        st["prev_note_on"][:] = (1, 0, 1)
        st["env"]["state"][0] = oracle.ENV_RELEASE
    m.set_state(st)
    assert m.state().tobytes() == st.tobytes()
    for v in range(V):
        fresh[v].load(st, v)
    S, E = lc.SPAN
    base, sbase = lc.base_image(V, 8), lc.base_image(V, 9)
    ref, rsync = base.copy(), sbase.copy()
    _uniform_ref(oracle, kind, fresh, S, E, ref, rsync, False, lc.SR, 220.0, True, kind.test_patch)
    out, sync = util.to_image(base), util.to_image(sbase)
    m.paint(zang.Span(S, E), [out, sync], [], False, _params(kind, m, kind.test_patch, freq=220.0, note_on=True))
    ctx.sync()
    _check(kind, m, out, sync, ref, rsync, fresh, "from a set state")
    if kind is lc.PORTA:
        assert int(m.state()["env"]["state"][0]) == oracle.ENV_RELEASE               # note_on while releasing, no new note: untouched
    m.close()


@both
def test_paints_span_paints_and_a_graph_replay_mix(oracle, kind):
    """a span paint, a captured span paint replayed twice and a plain paint of ONE object, in sequence == the reference (both images
    and the state); a single-stream capture"""
    import torch
    import zang_amd
    from zang_amd import zang
    V = 65
    tb = lc.tables(V, 5150)
    voices = kind.voices(oracle, V)
    base, sbase = lc.base_image(V, 8), lc.base_image(V, 9)
    ref, rsync = base.copy(), sbase.copy()
    for _ in range(3):
        lr.paint_spans(oracle, kind.paint, voices, tb, ref, rsync, lc.SPAN, lc.SR, False, kind.test_patch)
    _uniform_ref(oracle, kind, voices, *lc.SPAN, ref, rsync, False, lc.SR, 330.0, False, kind.test_patch)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        mg = kind.module()(V, c2)
        out, sync = util.to_image(base), util.to_image(sbase)
        tab = _table(mg, tb)
        tab.device(c2.device, list(lr.FIELDS))        # uploaded before the capture records
        span = zang.Span(*lc.SPAN)
        spans = lambda: mg.paint_spans(span, [out, sync], None, _params(kind, mg, kind.test_patch), tab)
        spans()
        g = c2.capture(spans)
        g.launch(); g.launch()
        mg.paint(span, [out, sync], [], False, _params(kind, mg, kind.test_patch, freq=330.0, note_on=False))
        c2.sync()
        _check(kind, mg, out, sync, ref, rsync, voices, "mixed")
        g.close(); mg.close()
        c2.close()


@both
def test_refusals(ctx, kind):
    import torch
    from zang_amd import abi, zang
    from zang_amd.runtime import as_buf
    V = 8
    tb = lc.tables(V, 1)
    m = kind.module()(V, ctx)
    paint, paint_spans = getattr(ctx.lib, f"zh_{kind.name}_paint"), getattr(ctx.lib, f"zh_{kind.name}_paint_spans")
    out, sync = ctx.image(lc.ROWS, V, fill=0.25), ctx.image(lc.ROWS, V, fill=0.5)
    before, sbefore = out.clone(), sync.clone()
    state = m.state().tobytes()
    span = zang.Span(*lc.SPAN)
    good = _params(kind, m, kind.test_patch)
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
    bad[abi.PORTA_SPAN_NOTE_ON] = abi.ScriptSpanParam(sp[abi.PORTA_SPAN_FREQ].f, None)   # `f` on a u-only field
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), bad, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    empty = abi.ScriptSpanTable(0, 0, ctb.count, ctb.start, ctb.end, ctb.note_id_changed)   # max_spans == 0
    assert paint_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(empty), 0) == abi.ZH_ERR_INVALID
    ctx.sync()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)) and torch.equal(sync.view(torch.int32), sbefore.view(torch.int32))
    assert m.state().tobytes() == state                                                   # nothing painted
    m.close()
