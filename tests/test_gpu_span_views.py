"""GPU: the SPAN paints on image views and in place -- zh_<module>_paint_spans of the ten builtin modules,
zh_script_module_paint_spans and the fused span voices -- against the oracle, bit for bit, with canaries around everything.

include/zang_hip.h promises two things about where images lie: a zh_buf is any device pointer with stride >= voices, and a paint
whose input or control image overlaps outputs[0] reads what zero-then-paint would read (an image that IS outputs[0] in the
reference's order: SineOsc and TriSawOsc read a frame's frequency after their own add, everything else before).
tests/test_gpu_views.py holds the plain paints to both; this file the span forms, in tests/paint_cases.py's geometries:

 - V = 68 and 130: the last wave of either has a few live lanes (blocks of 64);
 - 352 rows, span (13, 334): 321 frames, so every 8-frame chunk loop runs full chunks, its prefetch and its tail; the span starts
   and ends inside the image;
 - two carried buffers -- ADD onto random content, then ZERO_FIRST onto garbage -- of up to three sub-spans per voice.
"""
import os

import numpy as np
import pytest

from tests import module_spans_cases as msc
from tests import paint_cases as pc
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
FRAMES, SPAN = 352, (13, 334)
VS = [68, 130]
VIEW_GEOMETRIES = [g for g in pc.GEOMETRIES if g not in ("plain", "in_place")]
SMALL_GEOMETRIES = ["shifted", "odd_stride", "mixed_aligned", "params_shifted"]
# every image a module can take, given as an image
MODULE_IMAGES = {"sineosc": ("freq_img", "phase_img"), "pulseosc": ("freq_img",), "trisawosc": ("freq_img",), "filter": ("cut_img", "res_img")}


def _geo(name, V):
    return pc.Geometry(name, V, frames=FRAMES, span=SPAN)


def _no_nan(refs, what):
    for k, r in enumerate(refs):
        assert not np.isnan(r).any(), f"{what}: the reference of buffer {k} holds a NaN (bit equality would hide a difference)"


# ------------------------------------------------------------------------------------------------ a. builtin modules on views
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", VIEW_GEOMETRIES)
@pytest.mark.parametrize("name", list(msc.CASES))
def test_module_span_paints_on_views(ctx, oracle, name, geometry, V):
    """zh_<module>_paint_spans with the output, the module input, the cob images and the per-voice default arrays from a geometry:
    image columns and final state of every voice against the oracle, and nothing written outside view x span"""
    g = _geo(geometry, V)
    refs = msc._run(ctx, oracle, msc.CASES[name](), V, seed=V * 3 + len(name), mode="mix", images=MODULE_IMAGES.get(name, ()), nbuf=2, geo=g)
    _no_nan(refs, f"{name} [{geometry}]")


# ------------------------------------------------------------------------------------------------ b. builtin modules in place
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("name,which", msc.IN_PLACE)
def test_module_span_paints_in_place(ctx, oracle, name, which, V):
    """The image IS the output: ADD onto its own content, ZERO_FIRST (the paint reads the zeros), ADD again, against the oracle given
    one row for both.  The oracle run that reads a COPY of the row differs on bits, so a wrong order of read and add shows."""
    g = _geo("in_place", V)
    refs, copies = msc._run_in_place(ctx, oracle, msc.CASES[name](), V, seed=V + 17 * len(name + which), geo=g, which=which)
    _no_nan(refs, f"{name}, {which} is the output")
    lo, hi = SPAN
    differs = [not np.array_equal(a[:, lo:hi].view(np.uint32), b[:, lo:hi].view(np.uint32)) for a, b in zip(refs, copies)]
    assert differs[1], "reading the zeros of ZERO_FIRST and reading the image's old contents give the same bits: the case shows nothing"
    if (name, which) in (("sineosc", "freq_img"), ("trisawosc", "freq_img")):      # these read a frame's frequency AFTER their own add
        assert differs[0], "reading the frequency before and after the frame's own add give the same bits: the case shows nothing"


# ------------------------------------------------------------------------------------------------ c. script modules
_SCRIPTS = {}


def _script_program(ctx):
    from zang_amd import script
    if "prog" not in _SCRIPTS:
        text = open(os.path.join(ROOT, "tests", "golden", "script_modules.txt")).read()
        _SCRIPTS["prog"] = script.ScriptProgram(text, ctx, only=["Doubler", "Crush"], spans=True)
    return _SCRIPTS["prog"]


def _script_cases(g, V, x, rate, drive):
    """(module, the shared device params, voice -> the interpreter's) for an input image x ([V][FRAMES] host; None: the caller's)"""
    import torch
    gx = None if x is None else g.image("in", content=torch.from_numpy(np.ascontiguousarray(x.T)).cuda())
    grate, gdrive = g.per_voice(rate), g.per_voice(drive)
    return [("Doubler", "freq", {"sample_rate": SR, "freq": gx}, lambda v, xv: {"sample_rate": np.float32(SR), "freq": xv}),
            ("Crush", "input", {"sample_rate": SR, "input": gx, "rate": grate, "drive": gdrive},
             lambda v, xv: {"sample_rate": np.float32(SR), "input": xv, "rate": np.float32(rate[v]), "drive": np.float32(drive[v])})]


def _sub_spans(rng, V, same=False):
    """per voice 0-3 sub-spans inside SPAN from tests/test_gpu_script_spans.py's generator (same: one list for every voice)"""
    from tests.test_gpu_script_spans import _random_lists
    lists = _random_lists(rng, 1 if same else V, SPAN[1] - SPAN[0], [], vary=False)
    lists = [[(s + SPAN[0], e + SPAN[0], nic, vals) for s, e, nic, vals in spans] for spans in lists]
    return lists * V if same else lists


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", SMALL_GEOMETRIES)
def test_script_span_paints_on_views(ctx, geometry, V):
    """Doubler (a cob image) and Crush (stateful: Decimator into Distortion) through paint_spans, output and image parameter from
    different roles: two carried buffers (ADD onto random content, ZERO_FIRST onto garbage) against oracle/zs_interp.py per voice and
    sub-span"""
    from oracle import zangscript as zs, zs_interp
    from zang_amd import script, zang
    prog = _script_program(ctx)
    compiled = zs.compile(prog.text, prog.filename)
    g = _geo(geometry, V)
    s, e = SPAN
    rng = np.random.default_rng(V + 2)
    x = rng.uniform(-1, 1, (V, FRAMES)).astype(np.float32)
    rate = rng.uniform(-100, 60000, V).astype(np.float32); drive = rng.uniform(0, 1, V).astype(np.float32)
    for name, _, dev, host in _script_cases(g, V, x, rate, drive):
        m = prog.module(name, V, 0)
        voices = zs_interp.make_voices(compiled, name, V, 0)
        order = [p[0] for p in m.params]
        for b, zf in enumerate((False, True)):
            base = util.rng_buffers(V + 40 + b, V, FRAMES)
            out = g.image("out", content=util.to_image(base))
            ref = base.copy()
            if zf:
                ref[:, s:e] = 0.0
            lists = _sub_spans(rng, V)
            m.paint_spans(zang.Span(s, e), [out], script.ScriptSpanTable.from_lists(m.params, lists), dev, zero_first=zf)
            for v in range(V):
                hv = host(v, x[v])
                for (s0, e0, nic, _) in lists[v]:
                    voices[v].paint(s0, e0, ref[v], nic, [hv[n] for n in order])
            ctx.sync()
            assert ctx.last_form() == ["zs_paint_spans_" + name], ctx.last_form()
            util.assert_bitexact(util.from_image(out), ref, f"{name} [{geometry}] buffer {b} zf={zf}")
            _no_nan([ref], name)
            g.check_canaries(f"{name} buffer {b}")
            g.release([out])
        m.close()


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("name", ["Doubler", "Crush"])
def test_script_span_paints_in_place(ctx, name, V):
    """The image parameter IS the output, one table for every voice: ADD, then ZERO_FIRST (the paint reads the zeros), then ADD.  The
    reference is what the plain form does, which applies the rule already: zang.zero(span) for ZERO_FIRST, then one plain in-place
    ADD paint per sub-span with that sub-span's note_id_changed."""
    from zang_amd import script, zang
    prog = _script_program(ctx)
    s, e = SPAN
    rng = np.random.default_rng(V + 3)
    x = rng.uniform(-1, 1, (V, FRAMES)).astype(np.float32)
    rate = rng.uniform(-100, 60000, V).astype(np.float32); drive = rng.uniform(0, 1, V).astype(np.float32)
    g, g2 = _geo("in_place", V), _geo("in_place", V)
    outs = []
    for geo in (g, g2):
        outs.append(geo.image("out", content=util.to_image(x)))
    _, key, dev, _ = [c for c in _script_cases(g, V, None, rate, drive) if c[0] == name][0]
    _, _, dev2, _ = [c for c in _script_cases(g2, V, None, rate, drive) if c[0] == name][0]
    dev[key], dev2[key] = outs
    m, m2 = prog.module(name, V, 0), prog.module(name, V, 0)
    # Doubler: oracle/zs_interp.py given ONE row as output and parameter reproduces the plain form, and is the reference too.  (Crush:
    # the interpreter runs its two `out` statements as two passes over the span, the second reading what the first added; the
    # kernels read a frame once.  There the plain form alone is the reference: two GPU forms are compared.)
    from oracle import zangscript as zs, zs_interp
    interp = zs_interp.make_voices(zs.compile(prog.text, prog.filename), name, V, 0) if name == "Doubler" else None
    iref = x.copy()
    for b, zf in enumerate((False, True, False)):
        lists = _sub_spans(rng, V, same=True)
        if b < 2 and not any(e0 > s0 for s0, e0, _, _ in lists[0]):
            lists = [[(s + 5, e - 7, True, {})]] * V                    # (the first two paints paint something)
        m.paint_spans(zang.Span(s, e), [outs[0]], script.ScriptSpanTable.from_lists(m.params, lists), dev, zero_first=zf)
        ctx.sync()
        assert ctx.last_form() == (["k_elementwise"] if zf else []) + ["zs_paint_spans_" + name], ctx.last_form()
        if zf:
            zang.zero(zang.Span(s, e), outs[1], ctx=ctx)
        for (s0, e0, nic, _) in lists[0]:
            m2.paint(zang.Span(s0, e0), [outs[1]], None, nic, dev2)
        ctx.sync()
        ref = util.from_image(outs[1])
        _no_nan([ref], name)
        util.assert_bitexact(util.from_image(outs[0]), ref, f"{name} in place, paint {b} zf={zf}")
        if interp is not None:
            for v in range(V):
                if zf:
                    iref[v, s:e] = 0.0
                for (s0, e0, nic, _) in lists[v]:
                    interp[v].paint(s0, e0, iref[v], nic, [{"sample_rate": np.float32(SR), "freq": iref[v]}[n] for n, _, _ in m.params])
            util.assert_bitexact(ref, iref, f"{name} in place, paint {b}: the plain form against the interpreter")
        assert np.array_equal(m.get_state(), m2.get_state()), f"{name} in place: state after paint {b}"
        g.check_canaries(f"{name} in place, paint {b}")
    m.close(); m2.close()


# ------------------------------------------------------------------------------------------------ d. the fused span voices
VOICE_GEOMETRIES = ["shifted", "odd_stride", "mixed_aligned", "shared_allocation"]
from tests.test_gpu_curve_player import kits  # noqa: E402,F401  (the module-scoped kit fixture of the curve voice's own tests)


class _Voice:
    """One fused voice's "span paint equals the reference" scenario of its own test file, as what the driver below needs: rows,
    span, kernel, columns; start(ctx, oracle, V, kits) -> the module; tables(V, b); bases(V, b) -> (base, second base);
    reference(oracle, tb, ref, rsync or None, zero_first) painting both in place; paint(span, outs, tb, zero_first); check(...)"""
    columns = 2

    def close(self):
        self.m.close()


class _Lead(_Voice):
    def __init__(self, kind):
        from tests import lead_cases as lc
        self.kind, self.rows, self.span, self.kernel, self.lc = kind, lc.ROWS, lc.SPAN, "k_lead_spans", lc

    def start(self, ctx, oracle, V, kits):
        self.m, self.vs = self.kind.module()(V, ctx), self.kind.voices(oracle, V)

    def tables(self, V, b):
        return self.lc.tables(V, 1000 * V + b, note_on_first=b == 0)

    def bases(self, V, b):
        return self.lc.base_image(V, 77 + V + b), self.lc.base_image(V, 177 + V + b)

    def reference(self, oracle, tb, ref, rsync, zf):
        from tests import lead_reference as lr
        lr.paint_spans(oracle, self.kind.paint, self.vs, tb, ref, rsync, self.span, self.lc.SR, zf, self.kind.test_patch)

    def paint(self, span, outs, tb, zf):
        from tests import test_gpu_lead as t
        self.m.paint_spans(span, outs, None, t._params(self.kind, self.m, self.kind.test_patch), t._table(self.m, tb), zero_first=zf)

    def check(self, out, sync, ref, rsync, what):
        from tests import test_gpu_lead as t
        t._check(self.kind, self.m, out, sync, ref, rsync, self.vs, what)


class _HardSquare(_Lead):
    def __init__(self):
        from tests import lead_cases as lc
        self.rows, self.span, self.kernel, self.lc = lc.ROWS, lc.SPAN, "k_hard_square_spans", lc

    def start(self, ctx, oracle, V, kits):
        from tests import hard_square_cases as hq
        from zang_amd import modules as mod
        self.m, self.vs = mod.HardSquare(V, ctx), hq.voices(oracle, V)

    def reference(self, oracle, tb, ref, rsync, zf):
        from tests import hard_square_cases as hq
        hq.reference_spans(oracle, self.vs, tb, ref, rsync, zf)

    def paint(self, span, outs, tb, zf):
        from tests import hard_square_cases as hq, test_gpu_hard_square as t
        self.m.paint_spans(span, outs, None, self.m.Params(hq.SR), t._table(self.m, tb), zero_first=zf)

    def check(self, out, sync, ref, rsync, what):
        from tests import test_gpu_hard_square as t
        t._check(self.m, out, sync, ref, rsync, self.vs, what)


class _SawEnv(_Voice):
    columns = 1

    def __init__(self):
        from tests import test_gpu_saw_env as t
        self.t, self.rows, self.span, self.kernel = t, t.ROWS, t.SPAN, "k_saw_env_spans"

    def start(self, ctx, oracle, V, kits):
        from zang_amd import modules as mod
        self.m, self.vs = mod.SawEnv(V, ctx), self.t._voices(oracle, V)

    def tables(self, V, b):
        return self.t.tables(V, 1000 * V + b)

    def bases(self, V, b):
        return self.t.base_image(V, 77 + V + b), None

    def reference(self, oracle, tb, ref, rsync, zf):
        from tests import lead_reference as lr
        lr.paint_spans(oracle, self.t._paint, self.vs, tb, ref, None, self.span, self.t.SR, zf, None)

    def paint(self, span, outs, tb, zf):
        self.m.paint_spans(span, outs, None, self.m.Params(self.t.SR), self.t._table(self.m, tb), zero_first=zf)

    def check(self, out, sync, ref, rsync, what):
        self.t._check(self.m, out, ref, self.vs, what)


class _Detuned(_Voice):
    def __init__(self):
        from tests import detuned_cases as dc
        self.dc, self.rows, self.span, self.kernel = dc, dc.ROWS, dc.SPAN, "k_detuned_spans"

    def start(self, ctx, oracle, V, kits):
        from tests import test_gpu_detuned as t
        from zang_amd import modules as mod
        self.m, self.vs = mod.Detuned(V, ctx, self.dc.FIRST_SEED), t._voices(oracle, V)

    def tables(self, V, b):
        return self.dc.tables(V, 1000 * V + b, note_on_first=b == 0)

    def bases(self, V, b):
        return self.dc.base_image(V, 77 + V + b), self.dc.base_image(V, 177 + V + b)

    def reference(self, oracle, tb, ref, rsync, zf):
        from tests import detuned_reference as dr
        dr.paint_spans(oracle, self.vs, tb, ref, rsync, self.span, self.dc.SR, zf, self.dc.TEST_PATCH)

    def paint(self, span, outs, tb, zf):
        from tests import test_gpu_detuned as t
        self.m.paint_spans(span, outs, None, t._params(self.m, self.dc.TEST_PATCH), t._table(self.m, tb), zero_first=zf)

    def check(self, out, sync, ref, rsync, what):
        from tests import test_gpu_detuned as t
        t._check(self.m, out, sync, ref, rsync, self.vs, what)


class _Dual(_Voice):
    def __init__(self):
        from tests import test_gpu_dual as t
        self.t, self.rows, self.span, self.kernel = t, t.ROWS, t.SPAN, "k_dual_spans"

    def start(self, ctx, oracle, V, kits):
        from zang_amd import modules as mod
        self.m, self.vs = mod.Dual(V, ctx), self.t._voices(oracle, V)

    def tables(self, V, b):
        return self.t.tables(V, 1000 * V + b)

    def bases(self, V, b):
        return self.t.base_image(V, 77 + V + b), self.t.base_image(V, 177 + V + b)

    def reference(self, oracle, tb, ref, rsync, zf):
        from tests import two_reference as tr
        tr.paint_spans(oracle, self.vs, tb, ref, rsync, self.span, self.t.SR, zf, self.t.PATCH)

    def paint(self, span, outs, tb, zf):
        self.m.paint_spans(span, outs, None, self.m.Params(self.t.SR, patch=self.m.Patch(*self.t.PATCH)), self.t._table(self.m, tb), zero_first=zf)

    def check(self, out, sync, ref, rsync, what):
        self.t._check(self.m, (out, sync), (ref, rsync), self.vs, what)


class _CurvePlayer(_Voice):
    def __init__(self):
        from tests import curve_player_cases as cc
        self.cc, self.rows, self.span, self.kernel = cc, cc.ROWS, cc.SPAN, "k_curve_player_spans"

    def start(self, ctx, oracle, V, kits):
        from tests import curve_player_reference as cr
        from zang_amd import modules as mod
        self.kits = kits
        self.m, self.vs = mod.CurveVoice(V, ctx), [cr.Voice(oracle) for _ in range(V)]

    def tables(self, V, b):
        return self.cc.tables(V, 1000 * V + b, second=b == 1)

    def bases(self, V, b):
        return self.cc.base_image(V, 77 + V + b), self.cc.base_image(V, 177 + V + b)

    def reference(self, oracle, tb, ref, rsync, zf):
        from tests import curve_player_reference as cr
        r0, r1 = cr.paint_spans(oracle, self.kits[0], self.vs, tb, ref, rsync, self.span, self.cc.SR, zf)
        ref[:] = r0
        if rsync is not None:
            rsync[:] = r1

    def paint(self, span, outs, tb, zf):
        from tests import test_gpu_curve_player as t
        self.m.paint_spans(span, outs, None, self.m.Params(self.kits[1], self.cc.SR, 9.0, 99), t._table(self.m, tb), zero_first=zf)

    def check(self, out, sync, ref, rsync, what):
        from tests import test_gpu_curve_player as t
        t._check(self.m, [out] + ([] if sync is None else [sync]), [ref] + ([] if sync is None else [rsync]), self.vs, what)


def _lead(i):
    from tests import lead_cases as lc
    return _Lead(lc.KINDS[i])


# (name, the scenario, voices): one V of 68 or 130 each
VOICES = [("porta", lambda: _lead(0), 68), ("vibrato", lambda: _lead(1), 130), ("hard_square", _HardSquare, 130), ("saw_env", _SawEnv, 68),
          ("detuned", _Detuned, 130), ("dual", _Dual, 68), ("curve_player", _CurvePlayer, 130)]
VOICE_IDS = [v[0] for v in VOICES]


def _voice_on_views(ctx, oracle, kits, make, V, geometry, second):
    """two carried buffers, ADD then ZERO_FIRST, at the voice's own span: outputs[0] from role `out`, outputs[1] (second) from role
    `in` -- another stride and alignment; an ADD paint reads it through frame_loop's input path with its own stride"""
    from zang_amd import zang
    w = make()
    g = pc.Geometry(geometry, V, frames=w.rows, span=w.span)
    w.start(ctx, oracle, V, kits)
    second = second and w.columns == 2
    for b, zf in enumerate((False, True)):
        tb = w.tables(V, b)
        base, sbase = w.bases(V, b)
        ref, rsync = base.copy(), (sbase.copy() if second else None)
        w.reference(oracle, tb, ref, rsync, zf)
        out = g.image("out", content=util.to_image(base))
        sync = None
        if second:
            sync = g.image("in", content=util.to_image(sbase))
            g.writable("in")
        w.paint(zang.Span(*w.span), [out, sync] if second else [out], tb, zf)
        ctx.sync()
        assert ctx.last_form() == [w.kernel], ctx.last_form()
        w.check(out, sync, ref, rsync, f"[{geometry}] V={V} buffer {b} zf={zf}")
        _no_nan([ref] + ([rsync] if second else []), w.kernel)
        g.check_canaries(f"{w.kernel} buffer {b}")
        g.release([out] + ([sync] if second else []))
    w.close()


@pytest.mark.parametrize("geometry", VOICE_GEOMETRIES)
@pytest.mark.parametrize("name,make,V", VOICES, ids=VOICE_IDS)
def test_span_voices_on_views(ctx, oracle, kits, name, make, V, geometry):
    """every fused span voice with its columns views of a geometry, against its own reference, with canaries"""
    _voice_on_views(ctx, oracle, kits, make, V, geometry, True)


@pytest.mark.parametrize("name,make,V", [v for v in VOICES if v[0] != "saw_env"], ids=[v for v in VOICE_IDS if v != "saw_env"])
def test_two_column_span_voices_on_views_without_the_second_column(ctx, oracle, kits, name, make, V):
    _voice_on_views(ctx, oracle, kits, make, V, "odd_stride", False)
