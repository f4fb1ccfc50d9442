"""GPU: generated script modules painted from per-voice sub-span tables in one launch (zs_paint_spans_<name>,
zh_script_module_paint_spans) -- the reference's Trigger loop per voice (examples/example_script_runtime_poly.zig:146-164),
each sub-span one paint() call with its own note_id_changed and params, against oracle/zs_interp.py voice by voice, bit for
bit; against the lane kernel where every voice has one sub-span; through the polyphonic driver and the sequential mixdown;
in a captured graph; and the entry point's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import script_fuzz, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
F = 1024
MODULES = os.path.join(ROOT, "tests", "golden", "script_modules.txt")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example_script.txt")
CORPUS = ["Doubler", "Pluck", "CycleSine", "Bell", "Lead", "Hiss", "Buzz", "Crush", "Glide", "Sweep", "Maths", "Echo", "EchoLead",
          "Coin", "Jingle", "LateJingle", "Trig", "Shapes", "FilteredSawtooth", "FilteredSawtoothCtl", "HardSquare"]
RANGES = {"freq": (60.0, 3000.0), "phase": (-1.0, 1.0), "cut": (0.05, 0.9), "cutoff": (0.05, 0.9), "color": (-0.5, 1.0),
          "rate": (1000.0, 30000.0), "drive": (0.1, 3.0), "goal": (100.0, 1000.0), "freq_mul": (0.5, 2.0), "k": (0.5, 2.0),
          "echo_volume": (0.0, 0.9), "speed": (0.5, 2.0)}
SHAPE = [(0.0, 440.0), (0.0005, 880.0), (0.001, 110.0), (0.0016, 660.0)]


def _voices(V):
    """every voice up to 200; above, a stride sample and the voices at every wave edge in reach of it, first and last waves whole"""
    if V <= 200:
        return np.arange(V)
    edges = [e for w in range(0, V, 64) for e in (w, w + 63) if e < V and (w < 256 or w % 1024 == 0 or w + 64 >= V)]
    return np.unique(np.concatenate([np.arange(0, V, max(1, V // 160)), np.arange(64), np.arange(V - 64, V), edges]))


def _program(ctx, path, name):
    from zang_amd import script
    return script.ScriptProgram(open(path).read(), ctx, filename=os.path.basename(path), only=[name], spans=True)


def _random_lists(rng, V, F, spec, vary=True):
    """per voice 0-3 sub-spans in [0, F]: adjacent, gapped, empty, at the buffer's edges; random values per sub-span for every
    constant, cob constant, boolean and enum param (sample_rate stays the buffer's)"""
    out = []
    for v in range(V):
        c = int(rng.integers(0, 4))
        pts = np.sort(rng.integers(0, F + 1, 2 * c))
        if c and rng.random() < 0.3:
            pts[0] = 0
        if c and rng.random() < 0.3:
            pts[-1] = F
        spans = []
        for k in range(c):
            s, e = int(pts[2 * k]), int(pts[2 * k + 1])
            if k and rng.random() < 0.3:
                s = spans[-1][1]                                  # adjacent to the previous one
                e = max(e, s)
            vals = {}
            if vary:
                for name, kind, enum in spec:
                    if name == "sample_rate" or kind in ("buffer", "curve"):
                        continue
                    if kind == "boolean":
                        vals[name] = bool(rng.random() < 0.6)
                    elif kind == "one_of":
                        from zang_amd import zscript_native as native
                        labels = native.ENUM_LABELS[enum]
                        lab = labels[int(rng.integers(len(labels)))]
                        vals[name] = (lab, float(rng.uniform(0.001, 0.01))) if enum == "PaintCurve" and lab != "instantaneous" else (lab, None)
                    else:
                        lo, hi = RANGES.get(name, (0.1, 2.0))
                        vals[name] = float(np.float32(rng.uniform(lo, hi)))
            spans.append((s, e, bool(rng.random() < 0.4), vals))
        out.append(spans)
    return out


def _shared(rng, spec, V, F):
    """the paint's own params: a value for every param, images for waveforms ([V][F] host, uploaded by the caller)"""
    p = {}
    for name, kind, enum in spec:
        if name == "sample_rate":
            p[name] = np.float32(SR)
        elif kind == "buffer":
            lo, hi = (60.0, 3000.0) if name == "freq" else (-1.5, 1.5)
            p[name] = rng.uniform(lo, hi, (V, F)).astype(np.float32)
        elif kind == "curve":
            p[name] = SHAPE
        elif kind == "boolean":
            p[name] = True
        elif kind == "one_of":
            from zang_amd import zscript_native as native
            p[name] = (native.ENUM_LABELS[enum][1], 0.004 if enum == "PaintCurve" else None)
        else:
            lo, hi = RANGES.get(name, (0.1, 2.0))
            p[name] = np.float32((lo + hi) / 2)
    return p


def _interp_value(kind, value):
    if kind == "one_of" and isinstance(value, tuple):
        return value
    if kind == "boolean":
        return bool(value)
    if kind in ("constant", "constant_or_buffer") and not isinstance(value, np.ndarray):
        return np.float32(value)
    return value


def _interp_voices(text, filename, name, idx, first_seed):
    from oracle import zangscript as zs
    from oracle import zs_interp
    s = zs.compile(text, filename)
    mi = s.module_index(name)
    K = zs_interp.noise_field_count(s, mi)
    return {int(v): zs_interp.Instance(s, mi, iter(range(first_seed + int(v) * K, first_seed + (int(v) + 1) * K))) for v in idx}


def _device_params(shared):
    out = {}
    for k, v in shared.items():
        out[k] = util.to_image(v) if isinstance(v, np.ndarray) and v.ndim == 2 else (float(v) if isinstance(v, np.floating) else v)
    return out


def _parity(ctx, text, filename, name, V, seed, buffers=3, Fb=F):
    """buffers of random tables through paint_spans against zs_interp voice by voice (the voices of _voices(V)); then one
    ordinary paint must go on from the state the spans left"""
    import torch
    from zang_amd import script, zang
    prog = script.ScriptProgram(text, ctx, filename=filename, only=[name], spans=True)
    rng = np.random.default_rng(seed)
    try:
        m = prog.module(name, V, seed)
        spec = m.params
        kinds = {n: k for n, k, _ in spec}
        order = [n for n, _, _ in spec]
        idx = _voices(V)
        interp = _interp_voices(text, filename, name, idx, seed)
        for b in range(buffers + 1):
            shared = _shared(rng, spec, V, Fb)
            zf = b % 2 == 0
            base = rng.uniform(-1, 1, (V, Fb)).astype(np.float32)
            img = util.to_image(base)
            ref = base[idx].copy()
            last = b == buffers
            if last:                                                 # the lane kernel from the state the spans left
                nic = rng.random(V) < 0.3
                m.paint(zang.Span(0, Fb), [img], None, torch.from_numpy(nic.astype(np.uint8)).cuda(), _device_params(shared), zero_first=zf)
                for q, v in enumerate(idx):
                    if zf:
                        ref[q, :] = 0.0
                    interp[int(v)].paint(0, Fb, ref[q], bool(nic[v]), [_interp_value(kinds[n], shared[n]) if not (isinstance(shared[n], np.ndarray) and shared[n].ndim == 2)
                                                                        else shared[n][v] for n in order])
            else:
                per_voice = _random_lists(rng, V, Fb, spec)
                table = script.ScriptSpanTable.from_lists(spec, per_voice)
                m.paint_spans(zang.Span(0, Fb), [img], table, _device_params(shared), zero_first=zf)
                assert ctx.last_form() == ["zs_paint_spans_" + name]
                for q, v in enumerate(idx):
                    if zf:
                        ref[q, :] = 0.0
                    for (s, e, nic, vals) in per_voice[v]:
                        pv = []
                        for n in order:
                            x = vals.get(n, shared[n])
                            pv.append(x[v] if isinstance(x, np.ndarray) and x.ndim == 2 else _interp_value(kinds[n], x))
                        interp[int(v)].paint(s, e, ref[q], nic, pv)
            ctx.sync()
            got = util.from_image(img)[idx]
            util.assert_bitexact(got, ref, "%s V=%d seed %d buffer %d zf=%s%s" % (name, V, seed, b, zf, " (lane kernel after the spans)" if last else ""))
    finally:
        prog.close()


@pytest.mark.parametrize("name", CORPUS + ["DemoPlayer"])
def test_corpus_spans_equal_the_interpreter(ctx, name):
    path = EXAMPLE if name == "DemoPlayer" else MODULES
    for V in (1, 64, 65, 200):
        _parity(ctx, open(path).read(), os.path.basename(path), name, V, seed=V * 31 + len(name))


@pytest.mark.parametrize("name", ["Pluck", "Buzz", "Hiss", "Bell", "Echo", "Jingle", "DemoPlayer"])
def test_spans_at_4096_voices_equal_the_interpreter(ctx, name):
    path = EXAMPLE if name == "DemoPlayer" else MODULES
    _parity(ctx, open(path).read(), os.path.basename(path), name, 4096, seed=9, buffers=2)


@pytest.mark.parametrize("seed", range(30))
def test_random_scripts_spans_equal_the_interpreter(ctx, seed):
    text, name = script_fuzz.generate(seed)
    _parity(ctx, text, "fuzz", name, 70, seed, buffers=2, Fb=96)


def _one_span_each(ctx, name, V, seed):
    """every voice exactly one sub-span [s, e) with the shared params: the spans kernel and the lane kernel, same state, same bits"""
    import torch
    from zang_amd import script, zang
    prog = _program(ctx, EXAMPLE if name == "DemoPlayer" else MODULES, name)
    rng = np.random.default_rng(seed)
    try:
        a, b = prog.module(name, V, seed), prog.module(name, V, seed)
        spec = a.params
        for buf, (s, e, zf) in enumerate([(0, F, True), (100, 777, False), (5, 5, False), (0, 1000, True)]):
            shared = _shared(rng, spec, 1, F)
            for n, kind, _ in spec:
                if kind == "buffer":
                    shared[n] = torch.from_numpy(np.ascontiguousarray(rng.uniform(60, 3000, (F, V)).astype(np.float32))).cuda()
            dev = {k: (float(v) if isinstance(v, np.floating) else v) for k, v in shared.items()}
            nic = buf % 2 == 0
            base = torch.from_numpy(rng.uniform(-1, 1, (F, V)).astype(np.float32)).cuda()
            oa, ob = base.clone(), base.clone()
            a.paint(zang.Span(s, e), [oa], None, nic, dev, zero_first=zf)
            count = np.ones(V, np.uint32)
            table = script.ScriptSpanTable(spec, count, np.full((1, V), s), np.full((1, V), e), np.full((1, V), nic))
            b.paint_spans(zang.Span(s, e), [ob], table, dev, zero_first=zf)
            ctx.sync()
            assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), (name, V, buf)
            assert np.array_equal(a.get_state(), b.get_state()), (name, V, buf)
    finally:
        prog.close()


@pytest.mark.parametrize("name", ["Pluck", "Buzz", "Hiss", "Echo", "Jingle", "Sweep", "FilteredSawtooth", "DemoPlayer"])
def test_one_sub_span_per_voice_equals_the_lane_kernel(ctx, name):
    for V in (4096, 131072):
        _one_span_each(ctx, name, V, seed=5)


def _demo_events(rng, n_notes, seconds):
    """(t, note id, {freq, note_on}): note-ons at random times, each released a random time later"""
    ev = []
    for i in range(n_notes):
        t0 = float(rng.uniform(0, seconds)); dur = float(rng.uniform(0.002, seconds / 2))
        f = float(np.float32(rng.uniform(100, 1500)))
        ev.append((t0, i + 1, {"freq": f, "note_on": True}))
        ev.append((t0 + dur, i + 1, {"freq": f, "note_on": False}))
    ev.sort(key=lambda x: x[0])
    return ev


@pytest.mark.parametrize("polyphony,n_notes", [(8, 40), (1024, 1500)])
def test_poly_driver_and_sequential_mix_equal_the_reference_loop(ctx, polyphony, n_notes):
    """example_script_runtime_poly.zig's MainModule.paint over 8 buffers at 44,100 Hz: one paint_spans (zero first) and one sequential
    mixdown per buffer against the interpreter doing the reference's loop -- zero the temp over the sub-span, paint, addInto -- voice
    by voice in order, from the same schedule"""
    import torch
    from zang_amd import script, zang
    sr, Fb, B = 44100.0, 1024, 8
    rng = np.random.default_rng(polyphony)
    prog = _program(ctx, EXAMPLE, "DemoPlayer")
    try:
        m = prog.module("DemoPlayer", polyphony)
        events = _demo_events(rng, n_notes, B * Fb / sr)
        pv = script.PolyScriptVoice(m, polyphony, ["freq", "note_on"], events)
        interp = _interp_voices(open(EXAMPLE).read(), "example_script.txt", "DemoPlayer", range(polyphony), 0)
        img = ctx.image(Fb, polyphony)
        mix = torch.empty(Fb, dtype=torch.float32, device=img.device)
        temp = np.zeros(Fb, np.float32)
        painted = 0
        for b in range(B):
            table = pv.paint(zang.Span(0, Fb), [img], {"sample_rate": sr}, sr)
            zang.mixdownVoices(zang.Span(0, Fb), mix, img, zero_first=True, sequential=True)
            ref = np.zeros(Fb, np.float32)
            for v in range(polyphony):
                for k in range(int(table.count[v])):
                    s, e = int(table.start[k, v]), int(table.end[k, v])
                    temp[s:e] = 0.0
                    interp[v].paint(s, e, temp, bool(table.note_id_changed[k, v]),
                                    [np.float32(sr), np.float32(table.arrays["freq"][0][k, v]), bool(table.arrays["note_on"][1][k, v])])
                    ref[s:e] += temp[s:e]
                    painted += 1
            ctx.sync()
            assert np.array_equal(mix.cpu().numpy(), ref), (polyphony, b)
        assert painted > 2 * B and np.abs(ref).max() > 0
        pv.close()
    finally:
        prog.close()


def test_captured_spans_paint_replays_like_the_eager_call(ctx):
    import torch
    import zang_amd
    from zang_amd import script, zang
    V = 300
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        prog = _program(c2, MODULES, "Buzz")
        m = prog.module("Buzz", V)
        rng = np.random.default_rng(3)
        table = script.ScriptSpanTable.from_lists(m.params, _random_lists(rng, V, F, m.params))
        params = {"sample_rate": SR, "freq": 440.0, "color": 0.3, "note_on": True}
        m.paint_spans(zang.Span(0, F), [c2.image(F, V, fill=0.0)], table, params)     # (uploads the table: not inside the capture)
        c2.sync()
        st = m.get_state()
        oe, og = c2.image(F, V, fill=0.25), c2.image(F, V, fill=0.25)
        m.paint_spans(zang.Span(0, F), [oe], table, params)
        c2.sync()
        se = m.get_state()
        m.set_state(st)
        g = c2.capture(lambda: m.paint_spans(zang.Span(0, F), [og], table, params))
        assert any("zs_paint_spans_Buzz" in k for k in g.kernels())
        g.launch()
        c2.sync()
        assert torch.equal(oe.view(torch.int32), og.view(torch.int32))
        assert np.array_equal(se, m.get_state())
        g.close()
        prog.close()
        c2.close()


def test_form_and_refusals(ctx):
    import torch
    from zang_amd import abi, script, zang
    V = 70
    prog = _program(ctx, MODULES, "Buzz")
    plain = script.ScriptProgram(open(MODULES).read(), ctx, only=["Crush"], spans=True)
    lane_only = script.ScriptProgram(open(MODULES).read(), ctx, only=["Buzz"])
    try:
        m = prog.module("Buzz", V)
        out = ctx.image(F, V, fill=0.0)
        table = script.ScriptSpanTable(m.params, np.ones(V), np.zeros((1, V)), np.full((1, V), 10), np.zeros((1, V)))
        params = {"sample_rate": SR, "freq": 440.0, "color": 0.3, "note_on": True}
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0) == abi.ZH_OK
        assert ctx.last_form() == ["zs_paint_spans_Buzz"]
        assert m._paint_spans(zang.Span(0, F), [out], table, params, abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
        lm = lane_only.module("Buzz", V)
        assert lm._paint_spans(zang.Span(0, F), [out], table, params, 0) == abi.ZH_ERR_UNSUPPORTED
        idx = {n: i for i, (n, _, _) in enumerate(m.params)}
        f = torch.zeros(V, dtype=torch.float32, device=out.device); u = torch.zeros(V, dtype=torch.int32, device=out.device)

        def with_arrays(mod, name, use_f, use_u):
            sp = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
            sp[{n: i for i, (n, _, _) in enumerate(mod.params)}[name]] = abi.ScriptSpanParam(f.data_ptr() if use_f else None, u.data_ptr() if use_u else None)
            return sp
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0, with_arrays(m, "color", True, False)) == abi.ZH_OK
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0, with_arrays(m, "color", False, True)) == abi.ZH_ERR_INVALID   # u on a constant
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0, with_arrays(m, "note_on", True, False)) == abi.ZH_ERR_INVALID  # f on a boolean
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0, with_arrays(m, "note_on", False, True)) == abi.ZH_OK
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0, with_arrays(m, "freq", True, False)) == abi.ZH_OK          # a cob constant
        img = ctx.image(F, V, fill=440.0)
        pimg = dict(params, freq=img)
        assert m._paint_spans(zang.Span(0, F), [out], table, pimg, 0, with_arrays(m, "freq", True, False)) == abi.ZH_ERR_INVALID    # a cob image
        assert m._paint_spans(zang.Span(0, F), [out], table, params, 0, with_arrays(m, "freq", False, True)) == abi.ZH_ERR_INVALID   # u on a cob
        c = plain.module("Crush", V)
        cp = {"sample_rate": SR, "input": ctx.image(F, V, fill=0.5), "rate": 8000.0, "drive": 1.0}
        assert c._paint_spans(zang.Span(0, F), [out], table, cp, 0) == abi.ZH_OK
        assert c._paint_spans(zang.Span(0, F), [out], table, cp, 0, with_arrays(c, "input", True, False)) == abi.ZH_ERR_INVALID     # a waveform
        sweep = script.ScriptProgram(open(MODULES).read(), ctx, only=["Sweep"], spans=True).module("Sweep", V)
        sp_params = {"sample_rate": SR, "freq_mul": 1.0, "shape": SHAPE}
        assert sweep._paint_spans(zang.Span(0, F), [out], table, sp_params, 0, with_arrays(sweep, "shape", True, False)) == abi.ZH_ERR_INVALID  # a curve
        for field in ("count", "start", "end", "note_id_changed"):
            bad = script.ScriptSpanTable(m.params, np.ones(V), np.zeros((1, V)), np.full((1, V), 10), np.zeros((1, V)))
            tb, sp = bad.device(out.device, [n for n, _, _ in m.params])
            setattr(tb, field, None)
            ob = script.as_buf(out)
            arr = m._params(params, [])
            assert m.lib.zh_script_module_paint_spans(m.handle, 0, F, C.byref(ob), arr, len(m.params), sp, C.byref(tb), 0) == abi.ZH_ERR_INVALID, field
        tb, sp = table.device(out.device, [n for n, _, _ in m.params])
        tb.max_spans = 0
        assert m.lib.zh_script_module_paint_spans(m.handle, 0, F, C.byref(script.as_buf(out)), m._params(params, []), len(m.params), sp, C.byref(tb), 0) == abi.ZH_ERR_INVALID
        empty = prog.module("Buzz", 0)
        tb.max_spans = 1
        assert empty.lib.zh_script_module_paint_spans(empty.handle, 0, F, C.byref(script.as_buf(out)), m._params(params, []), len(m.params), sp, C.byref(tb), 0) == abi.ZH_OK
        ctx.sync()
    finally:
        prog.close(); plain.close(); lane_only.close()
