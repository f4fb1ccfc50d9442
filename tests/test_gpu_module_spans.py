"""GPU parity: the builtin modules over per-voice sub-span tables (zh_<module>_paint_spans) -- for every voice the reference's
Trigger loop (src/zang/trigger.zig:80-105), each sub-span one paint() call with its own note_id_changed and params, tags
included -- against the oracle painting voice by voice, one zo_<module>_paint per sub-span, bit for bit; against the plain
zh_<module>_paint where every voice has one full-buffer sub-span; HardSquareInstrument (examples/modules.zig:250-289) played
polyphonically through zh_poly_voice; captured graphs; and the entry points' refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import util
from tests.module_spans_cases import (CASES, K, F, SR, SamplerCase, _arrays, _defaults, _run, _tables)

pytestmark = pytest.mark.gpu


PARITY = [(n, V) for n in CASES for V in (1, 20, 64, 65, 200)] + [(n, 4096) for n in ("sineosc", "envelope", "filter", "sampler")]


@pytest.mark.parametrize("name,V", PARITY)
def test_oracle_parity(ctx, oracle, name, V):
    """Random 0-3 sub-spans per voice over 4 buffers, every span field random per sub-span (tags included), random
    note_id_changed, ADD and ZERO_FIRST: image and state bit-exact after every buffer."""
    case = CASES[name]()
    if name == "sampler":
        case.fmt = {1: 0, 20: 1, 64: 2, 65: 3, 200: 0, 4096: 1}[V]
    _run(ctx, oracle, case, V, seed=V * 7 + len(name))


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("mode", ["none", "mix"])
def test_fields_without_arrays(ctx, oracle, name, mode):
    """span_params NULL, and some fields as arrays with the others from the params (per-voice zh_f32 / zh_bool arrays)."""
    _run(ctx, oracle, CASES[name](), 97, seed=5 + len(name), mode=mode, nbuf=2)


@pytest.mark.parametrize("name,images", [("sineosc", ("freq_img",)), ("sineosc", ("phase_img",)), ("sineosc", ("freq_img", "phase_img")),
                                         ("pulseosc", ("freq_img",)), ("trisawosc", ("freq_img",)), ("filter", ("cut_img",)),
                                         ("filter", ("res_img",)), ("filter", ("cut_img", "res_img"))])
def test_cob_images_at_the_absolute_frame(ctx, oracle, name, images):
    """Cob images -- SineOsc frequency and phase, PulseOsc / TriSawOsc frequency (the controlled-frequency paths: TriSawOsc's f32
    phase, updated in place, and its end-of-paint wrap), Filter cutoff and resonance -- and the Filter's input are read at the
    absolute frame; the other fields vary per sub-span.  Image and state bit-exact after every buffer."""
    _run(ctx, oracle, CASES[name](), 130, seed=11 + len(images), images=images, nbuf=4)


def _sampler_variants():
    return [(fmt, ch) for fmt in (0, 1, 2, 3) for ch in (1, 2)]


@pytest.mark.parametrize("fmt,channels", _sampler_variants())
def test_sampler_formats(ctx, oracle, fmt, channels):
    """The four PCM formats, mono and stereo, loop on and off per sub-span, negative rates, note_id_changed resetting t."""
    case = SamplerCase()
    case.fmt, case.channels = fmt, channels
    _run(ctx, oracle, case, 150, seed=40 + fmt * 3 + channels, nbuf=3)


# ------------------------------------------------------------------ one full-buffer sub-span per voice == the plain paint
@pytest.mark.parametrize("V", [4096, 131072])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_sub_span_equals_plain_paint(ctx, name, V):
    """Every voice one sub-span [0, 1024) with the params of a plain paint (uniform tags): the same bits and state as
    zh_<module>_paint, which the rest of the suite pins against the oracle -- whatever form the plain paint takes."""
    import torch
    from zang_amd import zang
    case = CASES[name]()
    rng = np.random.default_rng(V + len(name))
    case.dflt = _defaults(case, rng, V)
    extra = {}
    gen = torch.Generator(device="cuda").manual_seed(V)
    if case.inputs:
        extra["input"] = torch.rand(F, V, generator=gen, device="cuda") * 2.0 - 1.0
    a, b = case.make(ctx, V), case.make(ctx, V)
    params = case.params(a, case.dflt, extra)
    nic_h = (rng.random(V) < 0.5).astype(np.uint8)
    nic = util.dev(nic_h)
    table = a.span_table(np.ones(V), np.zeros((1, V)), np.full((1, V), F), nic_h.reshape(1, V))
    for zf in (True, False):
        o1 = torch.rand(F, V, generator=gen, device="cuda") * 2.0 - 1.0
        o2 = o1.clone()
        a.paint(zang.Span(0, F), [o1], [], nic, params, zero_first=zf)
        b.paint_spans(zang.Span(0, F), [o2], None, params, table, zero_first=zf)
        ctx.sync()
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), (name, V, zf)
        if case.stateful:
            sa, sb = a.state(), b.state()
            assert sa.tobytes() == sb.tobytes(), (name, V, zf)
    a.close(); b.close()


# ------------------------------------------------------------------ heterogeneous voices in one launch
@pytest.mark.parametrize("name", ["filter", "envelope", "noise", "distortion"])
def test_heterogeneous_tags(ctx, oracle, name):
    """4,096 voices, one launch per buffer, random per-voice Filter types / Envelope curve tags / Noise colours / Distortion types."""
    _run(ctx, oracle, CASES[name](), 4096, seed=123, nbuf=2)


# ------------------------------------------------------------------ HardSquareInstrument, polyphonic
def test_hard_square_instrument_polyphony(ctx, oracle):
    """examples/modules.zig:250-289 at polyphony 8 over random notes, scheduled by zh_poly_voice: per buffer
    zh_pulseosc_paint_spans (freq per sub-span, color 0.5) into a zero-first temp, zh_gate_paint_spans (note_on per
    sub-span) into a second, zh_multiply over the buffer into a +0 output.  The oracle paints the same schedule voice by
    voice, one zo_hard_square_paint per sub-span.  Output and oscillator state bit-exact after every buffer."""
    import torch
    from zang_amd import abi, modules as mod, zang
    P, NB = 8, 24
    rng = np.random.default_rng(8)
    n_ev = 60
    t = np.sort(rng.uniform(0, NB * F / SR, n_ev)).astype(np.float32)
    rec = np.zeros(n_ev, np.dtype({"names": ["freq", "note_on"], "formats": ["<f4", "u1"], "offsets": [0, 4], "itemsize": 8}))
    ids = np.zeros(n_ev, np.uint64)
    live, nid = [], 1
    for i in range(n_ev):
        if live and rng.random() < 0.45:                         # a note off for a sounding note
            j = live.pop(int(rng.integers(0, len(live))))
            rec[i]["freq"], rec[i]["note_on"], ids[i] = j[1], 0, j[0]
        else:
            f = np.float32(110.0 * 2 ** (rng.integers(0, 36) / 12.0))
            rec[i]["freq"], rec[i]["note_on"], ids[i] = f, 1, nid
            live.append((nid, f)); nid += 1
    lib = ctx.lib
    h = C.c_void_p()
    abi.check(lib.zh_poly_voice_create(P, 8, 4, n_ev, rec.ctypes.data, t.ctypes.data, ids.ctypes.data, C.byref(h)), "zh_poly_voice_create")
    L = oracle.lib()
    sts = [oracle.HardSquare() for _ in range(P)]
    for s in sts:
        L.zo_hard_square_init(C.byref(s))
    osc, gate = mod.PulseOsc(P, ctx), mod.Gate(P, ctx)
    t0, t1 = ctx.image(F, P, fill=7.0), ctx.image(F, P, fill=7.0)
    tmp0 = np.zeros(F, np.float32); tmp1 = np.zeros(F, np.float32)
    painted = 0
    try:
        for b in range(NB):
            cap = 34
            count = np.zeros(P, np.uint32); start = np.zeros((cap, P), np.uint32); end = np.zeros((cap, P), np.uint32)
            prm = np.zeros((cap, P), rec.dtype); nic = np.zeros((cap, P), np.uint8)
            fr = np.array([F], np.uint32)
            abi.check(lib.zh_poly_voice_schedule(h, SR, fr.ctypes.data, 1, cap, count.ctypes.data, start.ctypes.data, end.ctypes.data,
                                                 prm.ctypes.data, nic.ctypes.data), "zh_poly_voice_schedule")
            Kb = max(int(count.max()), 1)
            painted += int(count.sum())
            freq = np.ascontiguousarray(prm["freq"][:Kb]); on = prm["note_on"][:Kb].astype(np.uint32)
            ref = np.zeros((P, F), np.float32)
            for v in range(P):
                for k in range(int(count[v])):
                    L.zo_hard_square_paint(C.byref(sts[v]), int(start[k, v]), int(end[k, v]), oracle.fptr(ref[v]), oracle.fptr(tmp0),
                                           oracle.fptr(tmp1), int(nic[k, v]), SR, float(freq[k, v]), int(on[k, v]))
            ot = osc.span_table(count, start[:Kb], end[:Kb], nic[:Kb], {"freq": (freq, None)})
            gt = gate.span_table(count, start[:Kb], end[:Kb], nic[:Kb], {"note_on": (None, on)})
            out = ctx.image(F, P, fill=0.0)
            sp = zang.Span(0, F)
            osc.paint_spans(sp, [t0], None, osc.Params(SR, zang.constant(440.0), 0.5), ot, zero_first=True)
            gate.paint_spans(sp, [t1], None, gate.Params(False), gt, zero_first=True)
            zang.multiply(sp, out, t0, t1, ctx)
            ctx.sync()
            util.assert_bitexact(util.from_image(out), ref, f"hard square buffer {b}")
            assert [int(x) for x in osc.state()["cnt"]] == [s.osc.cnt for s in sts], b
    finally:
        lib.zh_poly_voice_destroy(h)
    assert painted > NB * 2                                     # the schedule really played notes
    osc.close(); gate.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ capture
def test_captured_span_paints_replay_like_eager_calls(ctx):
    """A captured sequence of span paints (Envelope, Filter, SineOsc) replays like the same calls made eagerly."""
    import torch
    import zang_amd
    from zang_amd import zang
    V = 300
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        cases = [CASES["envelope"](), CASES["filter"](), CASES["sineosc"]()]
        rng = np.random.default_rng(4)
        bufs = _tables(V, 1, 5)
        count, start, end, nic = _arrays(bufs[0])
        inp = util.to_image(util.rng_buffers(6, V, F))
        mods, calls = [], []
        for case in cases:
            m = case.make(c2, V)
            case.dflt = _defaults(case, rng, V)
            arr = {n: g(rng, (K, V)) for n, g in case.fields}
            table = m.span_table(count, start, end, nic, arr)
            params = case.params(m, case.dflt, {"input": inp})
            mods.append(m)
            calls.append((m, params, table))
        oe = [c2.image(F, V, fill=0.25) for _ in cases]
        og = [c2.image(F, V, fill=0.25) for _ in cases]
        for (m, params, table), o in zip(calls, [c2.image(F, V, fill=0.0) for _ in cases]):
            m.paint_spans(zang.Span(0, F), [o], None, params, table)             # uploads the tables outside the capture
        c2.sync()
        st0 = [m.state() for m in mods]

        def seq(outs):
            for (m, params, table), o in zip(calls, outs):
                m.paint_spans(zang.Span(0, F), [o], None, params, table)
        seq(oe); seq(oe)
        c2.sync()
        se = [m.state() for m in mods]
        for m, s in zip(mods, st0):
            m.set_state(s)
        g = c2.capture(lambda: seq(og))
        kern = [k for k, _ in g.kernels()]
        assert {"k_envelope_spans", "k_filter_spans", "k_sineosc_spans"} <= set(kern), kern
        g.launch(); g.launch()
        c2.sync()
        for a, b in zip(oe, og):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for m, s in zip(mods, se):
            assert m.state().tobytes() == s.tobytes()
        g.close()
        for m in mods:
            m.close()
        c2.close()


def test_coalesced_capture_mixes_flagged_paints_and_span_paints(ctx):
    """ZH_CAPTURE_COALESCE: flagged constant-frequency zh_pulseosc_paint calls (held back, batched) mixed with
    zh_pulseosc_paint_spans on the same module replay like the eager sequence; the counters continue across both."""
    import torch
    import zang_amd
    from zang_amd import zang
    V = 256
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        case = CASES["pulseosc"]()
        rng = np.random.default_rng(12)
        m = case.make(c2, V)
        freq = util.dev(rng.uniform(100, 2000, V).astype(np.float32))
        params = m.Params(SR, zang.constant(freq), 0.3)
        case.dflt = _defaults(case, rng, V)
        count, start, end, nic = _arrays(_tables(V, 1, 13)[0])
        table = m.span_table(count, start, end, nic, {n: g(rng, (K, V)) for n, g in case.fields})
        sp = zang.Span(0, F)
        m.paint(sp, [c2.image(F, V, fill=0.0)], [], False, params)             # stores the constants a flagged paint reuses
        m.paint_spans(sp, [c2.image(F, V, fill=0.0)], None, params, table)      # (uploads the table)
        c2.sync()
        st0 = m.state()
        n_out = 7

        def seq(outs):
            m.paint(sp, [outs[0]], [], False, params, params_unchanged=True)
            m.paint(sp, [outs[1]], [], False, params, params_unchanged=True)
            m.paint_spans(sp, [outs[2]], None, params, table)
            m.paint(sp, [outs[3]], [], False, params, params_unchanged=True)
            m.paint_spans(sp, [outs[4]], None, params, table, zero_first=True)
            m.paint(sp, [outs[5]], [], False, params, params_unchanged=True)
            m.paint(sp, [outs[6]], [], False, params, params_unchanged=True)
        oe = [c2.image(F, V, fill=0.5) for _ in range(n_out)]
        og = [c2.image(F, V, fill=0.5) for _ in range(n_out)]
        seq(oe)
        c2.sync()
        se = m.state()
        m.set_state(st0)
        g = c2.capture(lambda: seq(og), coalesce=True)
        g.launch()
        c2.sync()
        for i, (a, b) in enumerate(zip(oe, og)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
        assert m.state().tobytes() == se.tobytes()
        # a second replay continues from where the first left the counters, like a second eager sequence
        oe2 = [c2.image(F, V, fill=0.5) for _ in range(n_out)]
        seq(oe2)
        c2.sync()
        se2 = m.state()
        m.set_state(se)
        og[:] = [o.fill_(0.5) for o in og]
        g.launch()
        c2.sync()
        for a, b in zip(oe2, og):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert m.state().tobytes() == se2.tobytes()
        g.close(); m.close(); c2.close()


# ------------------------------------------------------------------ refusals
def test_refusals(ctx):
    import torch
    from zang_amd import abi, zang
    V = 70
    sp0 = zang.Span(0, F)
    out = ctx.image(F, V, fill=0.0)
    f = torch.zeros(V * K, dtype=torch.float32, device=out.device)
    u = torch.zeros(V * K, dtype=torch.int32, device=out.device)
    count, start, end, nic = np.ones(V), np.zeros((1, V)), np.full((1, V), 10), np.zeros((1, V))

    def arrays(case, name, use_f, use_u):
        sp = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
        sp[[n for n, _ in case.fields].index(name)] = abi.ScriptSpanParam(f.data_ptr() if use_f else None, u.data_ptr() if use_u else None)
        return sp

    rng = np.random.default_rng(0)
    inp = ctx.image(F, V, fill=0.5)
    for name, case_t in CASES.items():
        case = case_t()
        m = case.make(ctx, V)
        case.dflt = _defaults(case, rng, V)
        params = case.params(m, case.dflt, {"input": inp})
        table = m.span_table(count, start, end, nic)
        assert m._paint_spans(sp0, [out], None, params, table, 0) == abi.ZH_OK, name
        assert ctx.last_form() == ["k_%s_spans" % name], (name, ctx.last_form())
        assert m._paint_spans(sp0, [out], None, params, table, abi.PAINT_PARAMS_UNCHANGED) == abi.ZH_OK, name
        assert m._paint_spans(sp0, [out], None, params, table, abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED, name
        kinds = {"constant": (True, False), "boolean": (False, True), "tag": (False, True), "curve": (True, True)}
        for fname, kind in m._span_fields:
            ok_f, ok_u = kinds[kind]
            assert m._paint_spans(sp0, [out], None, params, table, 0, arrays(case, fname, True, False)) == (abi.ZH_OK if ok_f else abi.ZH_ERR_INVALID), (name, fname)
            assert m._paint_spans(sp0, [out], None, params, table, 0, arrays(case, fname, False, True)) == (abi.ZH_OK if ok_u else abi.ZH_ERR_INVALID), (name, fname)
        # NULL params, NULL table arrays, max_spans == 0
        tb, sp = table.device(out.device, [n for n, _ in m._span_fields])
        fn = getattr(m.lib, "zh_%s_paint_spans" % name)
        ob = (abi.Buf * 1)(zang.as_buf(out))
        cp = m._cparams(params)
        assert fn(m.handle, 0, F, ob, None, None, sp, C.byref(tb), 0) == abi.ZH_ERR_INVALID, name
        for field in ("count", "start", "end", "note_id_changed"):
            tb2, _ = table.device(out.device, [n for n, _ in m._span_fields])
            setattr(tb2, field, None)
            assert fn(m.handle, 0, F, ob, None, C.byref(cp), sp, C.byref(tb2), 0) == abi.ZH_ERR_INVALID, (name, field)
        tb.max_spans = 0
        assert fn(m.handle, 0, F, ob, None, C.byref(cp), sp, C.byref(tb), 0) == abi.ZH_ERR_INVALID, name
        m.close()
        # no voices: ZH_OK, nothing runs
        e = case.make(ctx, 0)
        tb.max_spans = 1
        assert getattr(e.lib, "zh_%s_paint_spans" % name)(e.handle, 0, F, ob, None, C.byref(cp), sp, C.byref(tb), 0) == abi.ZH_OK, name
        e.close()
    # a span array on a cob whose tag is BUFFER
    img = ctx.image(F, V, fill=440.0)
    s = CASES["sineosc"]()
    m = s.make(ctx, V)
    s.dflt = _defaults(s, rng, V)
    table = m.span_table(count, start, end, nic)
    p = s.params(m, s.dflt, {"freq_img": img})
    assert m._paint_spans(sp0, [out], None, p, table, 0) == abi.ZH_OK
    assert m._paint_spans(sp0, [out], None, p, table, 0, arrays(s, "freq", True, False)) == abi.ZH_ERR_INVALID
    assert m._paint_spans(sp0, [out], None, p, table, 0, arrays(s, "phase", True, False)) == abi.ZH_OK
    m.close()
    fc = CASES["filter"]()
    m = fc.make(ctx, V)
    fc.dflt = _defaults(fc, rng, V)
    p = fc.params(m, fc.dflt, {"input": inp, "cut_img": img})
    assert m._paint_spans(sp0, [out], None, p, table, 0, arrays(fc, "cutoff", True, False)) == abi.ZH_ERR_INVALID
    assert m._paint_spans(sp0, [out], None, p, table, 0, arrays(fc, "res", True, False)) == abi.ZH_OK
    m.close()
    for pn in ("pulseosc", "trisawosc"):
        pc = CASES[pn]()
        m = pc.make(ctx, V)
        pc.dflt = _defaults(pc, rng, V)
        p = m.Params(SR, zang.buffer(img), 0.5)
        assert m._paint_spans(sp0, [out], None, p, table, 0) == abi.ZH_OK
        assert m._paint_spans(sp0, [out], None, p, table, 0, arrays(pc, "freq", True, False)) == abi.ZH_ERR_INVALID
        assert m._paint_spans(sp0, [out], None, p, table, 0, arrays(pc, "color", True, False)) == abi.ZH_OK
        m.close()
    # tags out of range in params
    for name, bad in (("filter", lambda c, p: setattr(p, "type", 6)), ("distortion", lambda c, p: setattr(p, "type", 2)),
                      ("noise", lambda c, p: setattr(p, "color", 2)), ("envelope", lambda c, p: setattr(p.attack, "tag", 4))):
        c = CASES[name]()
        m = c.make(ctx, V)
        c.dflt = _defaults(c, rng, V)
        p = c.params(m, c.dflt, {"input": inp})
        cp = m._cparams(p)
        bad(c, cp)
        tb, sp = table.device(out.device, [n for n, _ in m._span_fields])
        ob = (abi.Buf * 1)(zang.as_buf(out))
        assert getattr(m.lib, "zh_%s_paint_spans" % name)(m.handle, 0, F, ob, None, C.byref(cp), sp, C.byref(tb), 0) == abi.ZH_ERR_INVALID, name
        m.close()
    ctx.sync()


@pytest.mark.parametrize("name", ["pulseosc", "trisawosc"])
def test_flagged_paint_after_a_span_paint_recomputes_its_constants(ctx, name):
    """ZH_PAINT_PARAMS_UNCHANGED promises the params of the module's previous paint.  A span paint is that previous paint: after
    paint(freq array P holding X), paint_spans(P now holding Y), a flagged paint(P, Y) must give what an unflagged one gives --
    not the constants the table still holds for X."""
    import torch
    from zang_amd import zang
    V = 256
    case = CASES[name]()
    rng = np.random.default_rng(31)
    x = rng.uniform(100, 2000, V).astype(np.float32)
    y = rng.uniform(100, 2000, V).astype(np.float32)
    sp = zang.Span(0, F)
    outs = []
    for flagged in (True, False):
        m = case.make(ctx, V)
        freq = util.dev(x)
        params = m.Params(SR, zang.constant(freq), 0.3)
        table = m.span_table(np.ones(V), np.zeros((1, V)), np.full((1, V), F), np.zeros((1, V)))
        o = [ctx.image(F, V, fill=0.0) for _ in range(3)]
        m.paint(sp, [o[0]], [], False, params)                      # stores the constants of X
        freq.copy_(torch.from_numpy(y))
        m.paint_spans(sp, [o[1]], None, params, table)
        m.paint(sp, [o[2]], [], False, params, params_unchanged=flagged)
        ctx.sync()
        outs.append((o[2], m.state()))
        m.close()
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert outs[0][1].tobytes() == outs[1][1].tobytes()
