"""GPU: paints on image VIEWS -- odd strides, misaligned bases, images of one call with different strides, disjoint views of one
allocation, in-place -- against the oracle, bit for bit, with canaries around everything.

The C ABI lets a zh_buf be any device pointer with stride >= voices (include/zang_hip.h), and a host uses that: several instruments
share one [frames][instruments x voices] image.  tests/paint_cases.py holds the per-module oracle drivers and the geometries (its
docstring has the table); here every case runs in every geometry but `plain` (tests/test_gpu_dispatch.py runs that one):

 - V = 256 (a multiple of 4 and of 64: every 16-byte form's voice-count condition holds, so only the pointer and stride gates stand
   between a misaligned view and a vector access) and V = 68 (a multiple of 4 whose second wave has four live lanes);
 - 352 rows, span (13, 334): 321 frames -- at least 128, so the frame-range forms split it; at least 64, so the wave pipelines take
   it (ten 32-frame tiles); no multiple of 8, so every chunk loop runs its tail; it starts and ends inside the image;
 - forms: `default` (every ZH_ variable cleared), `walks` (every *_ranges row 0 and every *_pc*_max / *_ring_max / *_pipe_max /
   delay_frames_max row 0: the lane-per-voice forms large voice counts take) and `rows` (the chunked Distortion and elementwise
   kernels forced at a small voice count, and the kernel that ran asserted: the canaries alone cannot tell "gate right" from "fast
   path never taken").
"""
import os
import re

import numpy as np
import pytest

from tests import mix_groups_cases as mg
from tests import mix_order_reference as mo
from tests import paint_cases as pc
from tests import util
from tests.test_gpu_basics import OPS, _gpu_op, _oracle_op

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
FRAMES, SPAN, DELAY = 352, (13, 334), 100
VS = [256, 68]
VIEW_GEOMETRIES = [g for g in pc.GEOMETRIES if g != "plain"]
SMALL_GEOMETRIES = ["shifted", "odd_stride", "mixed_aligned", "params_shifted"]
# every image of these is 16-byte aligned in every row (shared_allocation: columns 4, V + 12, 2 V + 20 of rows 3 V + 24 apart)
ALIGNED = {"plain", "mixed_aligned", "params_shifted", "shared_allocation"}


# ... and these have a 16-byte aligned OUTPUT in every row (what a kernel that only writes 16 bytes at a time needs)
OUT_ALIGNED = ALIGNED | {"in_misaligned"}


def _geo(name, V):
    return pc.Geometry(name, V, frames=FRAMES, span=SPAN, delay_samples=DELAY)


def _clear_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("ZH_") and name not in ("ZH_ENV_LIVE",):
            monkeypatch.delenv(name)                           # default dispatch, whatever the suite was started with


def _walk_rows():
    """the rows that switch the frame-range forms and the wave pipelines off, from the library's table by name (a new row joins)"""
    from tests.test_gpu_dispatch import _table_rows
    pat = re.compile(r"(_ranges|_pc\w*_max|_ring_max|_pipe_max)$|^delay_frames_max$")
    return sorted(n for n in _table_rows() if pat.search(n))


WALK_ROWS = _walk_rows()


def _set_forms(monkeypatch, forms):
    _clear_env(monkeypatch)
    if forms == "walks":
        util.set_form(monkeypatch, **{n: 0 for n in WALK_ROWS})
    elif forms == "rows":
        util.set_form(monkeypatch, basics_rows_min=0, distortion_rows_min=0)


def _run_cases(ctx, oracle, geometry, V, names, cutoff_in_place=True):
    g = _geo(geometry, V)
    sh = pc.Shared(ctx, V, np.arange(V, dtype=np.int64), g)
    g.check_canaries("the shared inputs")
    for name in names:
        pc.CASES[name](ctx, oracle, sh)                        # (each case ends with the canary check: Shared.finish)
    if geometry == "in_place" and cutoff_in_place:             # Filter once more, painting onto its cutoff image
        sh.alias_ctl = True
        pc.CASES["filter_notch_image"](ctx, oracle, sh)
    return sh


# ------------------------------------------------------------------------------------------------ the main test
@pytest.mark.parametrize("forms", ["default", "walks"])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", VIEW_GEOMETRIES)
def test_paint_views_equal_the_oracle(ctx, oracle, geometry, V, forms, monkeypatch):
    """Every case of tests/paint_cases.py (in_place: those that read an image), every voice against the oracle bit for bit -- image
    columns and final states -- and nothing written outside view x span: guards, rows outside the span, padding columns, the other
    images and the per-voice arrays with their guard elements."""
    _set_forms(monkeypatch, forms)
    sh = _run_cases(ctx, oracle, geometry, V, pc.IMAGE_CASES if geometry == "in_place" else list(pc.CASES))
    # The hardware carries out a misaligned 16-byte global access, so the bits alone do not show a missing pointer gate: the kernel
    # that ran is asserted too.  V is a multiple of 4, so the 16-byte form runs exactly where everything it accesses 16 bytes at a
    # time is aligned: Gate its output; the constant-frequency oscillators their output and the per-voice freq / color arrays.
    want = {"Gate": "k_gate4" if geometry in OUT_ALIGNED else "k_gate"}
    for name in ("pulse osc const", "trisaw osc const"):
        want[name] = "k_osc_const4" if geometry in OUT_ALIGNED and geometry != "params_shifted" else "k_osc_const"
    for name, kernel in want.items():
        if name in sh.forms:
            assert sh.forms[name] == [kernel], (geometry, name, sh.forms[name])


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", list(pc.GEOMETRIES))
def test_paint_views_chunked_distortion_is_taken_exactly_where_the_rows_allow(ctx, oracle, geometry, V, monkeypatch):
    """forms = rows: k_distortion_chunks (16-byte accesses to the output and the input) forced at a small voice count.  With every row
    of both images 16-byte aligned it is the kernel that ran; with a misaligned base or an odd stride it is not -- and either way the
    bits are the oracle's and the canaries stand."""
    _set_forms(monkeypatch, "rows")
    _run_cases(ctx, oracle, geometry, V, ["stateless"], cutoff_in_place=False)
    assert ctx.last_form() == (["k_distortion_chunks"] if geometry in ALIGNED else ["k_distortion"]), (geometry, ctx.last_form())
    util.set_form(monkeypatch, distortion_rows_min=1 << 30)
    _run_cases(ctx, oracle, geometry, V, ["stateless"], cutoff_in_place=False)
    assert ctx.last_form() == ["k_distortion"], ctx.last_form()


# ------------------------------------------------------------------------------------------------ basics
SCALAR_OPS = {"set", "addScalar", "addScalarInto", "multiplyScalar", "multiplyWithScalar"}


@pytest.mark.parametrize("rows", [False, True], ids=["default", "rows"])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", SMALL_GEOMETRIES)
def test_basics_on_views(ctx, oracle, geometry, V, rows, monkeypatch):
    """every operation of basics.zig with dest / a / b from the three image roles and a per-voice scalar, as test_basics_bitexact
    compares them; the float4 kernels run exactly where every pointer the operation uses allows them"""
    import torch
    from zang_amd import zang
    _set_forms(monkeypatch, "rows" if rows else "default")
    g = _geo(geometry, V)
    s, e = SPAN
    dest = util.rng_buffers(1, V, FRAMES); a = util.rng_buffers(2, V, FRAMES); b = util.rng_buffers(3, V, FRAMES)
    sc = np.random.default_rng(4).uniform(-2, 2, V).astype(np.float32)
    ga = g.image("in", content=torch.from_numpy(np.ascontiguousarray(a.T)).cuda())
    gb = g.image("ctl", content=torch.from_numpy(np.ascontiguousarray(b.T)).cuda())
    gsc = g.per_voice(sc)
    for name in OPS:
        ref = dest.copy()
        _oracle_op(oracle, name, s, e, ref, a, b, sc)
        gd = g.image("out", content=torch.from_numpy(np.ascontiguousarray(dest.T)).cuda())
        _gpu_op(ctx, name, zang.Span(s, e), gd, ga, gb, gsc)
        ctx.sync()
        vec = geometry in ALIGNED and not (geometry == "params_shifted" and name in SCALAR_OPS)
        assert ctx.last_form() == ["k_elementwise_chunks" if vec and rows else "k_elementwise"], (name, ctx.last_form())
        util.assert_bitexact(util.from_image(gd)[:, s:e], ref[:, s:e], f"{name} [{geometry}]")
        g.check_canaries(name)
        g.release([gd])


# ------------------------------------------------------------------------------------------------ mixdowns
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", SMALL_GEOMETRIES)
def test_mixdown_voices_from_a_view(ctx, geometry, V):
    """zh_mixdown_voices from a view into a row that starts at element 1: the tree form against an f64 sum (the sqrt(V) * eps bound of
    test_mixdown_voices), ZH_MIX_SEQUENTIAL against the f32 adds in voice order, bit for bit; the row outside the span stays"""
    import torch
    from zang_amd import zang
    g = _geo(geometry, V)
    s, e = SPAN
    src = util.rng_buffers(9, V, FRAMES)
    img = g.image("in", content=torch.from_numpy(np.ascontiguousarray(src.T)).cuda())
    for sequential in (False, True):
        full = torch.full((FRAMES + 2,), 0.5, dtype=torch.float32, device="cuda")
        mix = full[1:1 + FRAMES]
        assert mix.data_ptr() % 16 == 4
        zang.mixdownVoices(zang.Span(s, e), mix, img, sequential=sequential, ctx=ctx)
        ctx.sync()
        got = full.cpu().numpy()
        assert np.array_equal(got[:1 + s], np.full(1 + s, 0.5, np.float32)) and np.array_equal(got[1 + e:], np.full(FRAMES + 1 - e, 0.5, np.float32))
        got = got[1:1 + FRAMES]
        if sequential:
            ref = np.full(FRAMES, 0.5, np.float32)
            for v in range(V):                                 # out += voice_v, in order
                ref[s:e] = ref[s:e] + src[v, s:e]
            util.assert_bitexact(got, ref, "sequential mix")
        else:
            ref = 0.5 + src.astype(np.float64).sum(axis=0)
            bound = 4 * np.sqrt(V) * np.finfo(np.float32).eps * np.abs(src).astype(np.float64).sum(axis=0).max()
            assert np.abs(got[s:e] - ref[s:e]).max() <= bound
            # ... and the tree order itself, bit for bit (tests/mix_order_reference.py)
            util.assert_bitexact(got, mo.tree_mix_span(src, np.full(FRAMES, 0.5, np.float32), s, e, False), f"tree order [{geometry}]")
        g.check_canaries("mixdown")


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", SMALL_GEOMETRIES)
def test_grouped_mixdown_from_a_view(ctx, oracle, geometry, V):
    """zh_mixdown_groups and zh_mixdown_groups_pcm (s16, two channels, channel 1) with the source a view and dst / acc rows of wider
    tensors, against tests/mix_groups_cases.py bit for bit; the other channel's bytes and the rows' padding stay"""
    import torch
    from zang_amd import zang
    g = _geo(geometry, V)
    P, G, VOL = 4, V // 4, 0.25
    rng = np.random.default_rng(V)
    img = mg.image(rng, FRAMES, V, scale=2.5)
    start = mg.image(rng, FRAMES, G, special_rate=0.004).T.copy()
    src = g.image("in", content=torch.from_numpy(img).cuda())
    for zero_first in (False, True):
        wide = torch.full((G, FRAMES + 5), 7.0, dtype=torch.float32, device="cuda")
        dst = wide[:, 1:1 + FRAMES]
        dst.copy_(torch.from_numpy(start))
        zang.mixdownGroups(zang.Span(*SPAN), dst, src, P, zero_first=zero_first, ctx=ctx)
        ctx.sync()
        got = wide.cpu().numpy()
        assert mg.same_f32(got[:, 1:1 + FRAMES], mg.ref_sums(img, P, start, SPAN, zero_first)), zero_first
        assert (got[:, :1] == 7.0).all() and (got[:, 1 + FRAMES:] == 7.0).all()
    nch, ch, bps = 2, 1, 2
    prefill = rng.integers(0, 256, (G, FRAMES * nch * bps), dtype=np.uint8)
    for use_acc in (True, False):
        sums = mg.ref_sums(img, P, start, SPAN, not use_acc)
        want = mg.ref_pcm(oracle, sums, SPAN, True, nch, ch, VOL, prefill)
        wide = torch.full((G, FRAMES * nch * bps + 6), 0x5a, dtype=torch.uint8, device="cuda")
        dst = wide[:, 2:2 + FRAMES * nch * bps]
        dst.copy_(torch.from_numpy(prefill))
        accw = torch.full((G, FRAMES + 3), 7.0, dtype=torch.float32, device="cuda")
        acc = accw[:, 1:1 + FRAMES]
        acc.copy_(torch.from_numpy(start))
        zang.mixdownGroupsPcm(zang.Span(*SPAN), dst, src, P, 1, nch, ch, VOL, acc=acc if use_acc else None, ctx=ctx)
        ctx.sync()
        got = wide.cpu().numpy()
        body = got[:, 2:2 + FRAMES * nch * bps]
        assert np.array_equal(body, want), (use_acc, int((body != want).sum()))
        other = np.ones((FRAMES, nch, bps), bool); other[:, ch, :] = False
        assert np.array_equal(body[:, other.reshape(-1)], prefill[:, other.reshape(-1)])          # the other channel's bytes
        assert (got[:, :2] == 0x5a).all() and (got[:, 2 + FRAMES * nch * bps:] == 0x5a).all()      # the rows' padding
        assert mg.same_f32(accw.cpu().numpy()[:, 1:1 + FRAMES], start) and (accw.cpu().numpy()[:, :1] == 7.0).all()
    g.check_canaries("grouped mixdown")


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", SMALL_GEOMETRIES)
def test_nice_fused_mixdown_into_rows_at_element_1(ctx, oracle, geometry, V):
    """NiceInstrument.paint_mix / paint_mix_stereo with the mix rows sliced at element 1 and the per-voice arrays from the geometry,
    against the per-voice paint summed in f64 (the bound of test_nice_paint_mix: 4 * sqrt(V) * eps * the largest sum of magnitudes),
    and against the documented summation order of that paint, bit for bit (tests/mix_order_reference.py)"""
    import torch
    from zang_amd import modules as mod, zang, workloads
    g = _geo(geometry, V)
    s, e = SPAN
    freq, color, u2, _ = workloads.voice_params(5, 7, V)
    gl = (0.5 + 0.5 * (2.0 * u2 - 1.0)).astype(np.float32); gr = (1.0 - gl).astype(np.float32)
    gc, gf, dgl, dgr = g.per_voice(color), g.per_voice(freq), g.per_voice(gl), g.per_voice(gr)
    m1, m2, m3 = (mod.NiceInstrument(V, gc, ctx) for _ in range(3))
    rows_per = mo.rows_per_for(V, ctx.forms()["nice_mix_wg_min"][1])
    for k, (on, nic) in enumerate(((True, True), (False, False))):
        per_voice = g.image("out", fill=0.0)
        P = m1.Params(SR, gf, on)
        m1.paint(zang.Span(s, e), [per_voice], None, nic, P)
        rows = torch.full((3, FRAMES + 2), 0.25, dtype=torch.float32, device="cuda")
        mono, left, right = rows[0, 1:1 + FRAMES], rows[1, 1:1 + FRAMES], rows[2, 1:1 + FRAMES]
        m2.paint_mix(zang.Span(s, e), mono, nic, P)
        m3.paint_mix_stereo(zang.Span(s, e), left, right, dgl, dgr, nic, P)
        ctx.sync()
        pv = per_voice.cpu().numpy().astype(np.float64)                # [frames][voices]
        got = rows.cpu().numpy()
        for r, gain in ((0, None), (1, gl), (2, gr)):
            terms = pv if gain is None else (per_voice.cpu().numpy() * gain[None, :]).astype(np.float64)      # the products are f32
            ref = 0.25 + terms.sum(axis=1)
            bound = 4 * np.sqrt(V) * np.finfo(np.float32).eps * max(np.abs(terms).sum(axis=1).max(), 1.0)
            assert np.abs(got[r, 1 + s:1 + e] - ref[s:e]).max() <= bound, (k, r)
            assert (got[r, :1 + s] == 0.25).all() and (got[r, 1 + e:] == 0.25).all(), (k, r)
        quarter = np.full(FRAMES, 0.25, np.float32)                    # ... and the summation order itself, every frame
        util.assert_bitexact(got[0, 1:1 + FRAMES], mo.fused_mix_span(per_voice.cpu().numpy(), None, quarter, s, e, False, rows_per), f"mono order, paint {k}")
        for r, want in zip((1, 2), mo.fused_mix_span(per_voice.cpu().numpy(), (gl, gr), (quarter, quarter), s, e, False, rows_per)):
            util.assert_bitexact(got[r, 1:1 + FRAMES], want, f"stereo order, paint {k} channel {r - 1}")
        assert float(np.abs(pv).max()) > 0.01 or k == 1
        g.check_canaries("nice mix")
        g.release([per_voice])
    assert np.array_equal(m1.state(), m2.state()) and np.array_equal(m1.state(), m3.state())


# ------------------------------------------------------------------------------------------------ oscillator batches
@pytest.mark.parametrize("variant", ["same", "one_stride_differs", "one_shifted"])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("kind", ["pulse", "trisaw"])
def test_osc_batch_on_views(ctx, oracle, kind, V, variant):
    """paint_batch with three buffers: all in the mixed_aligned output geometry; or one of them with another stride, (still 16-byte aligned), or with a base
    4 bytes past its alignment (osc.hip's route for batches whose outputs differ) -- every buffer and the counters against the oracle"""
    from tests.test_gpu_osc import _oracle_buffers
    from zang_amd import modules as mod, zang, workloads
    freq, color, _, _ = workloads.voice_params(2, 7, V)
    freq[:3] = [6000.5, -1.0, 440.0]
    ref, rcnt = _oracle_buffers(oracle, kind, V, FRAMES, SPAN, 3, freq, color)
    odd = {"same": "mixed_aligned", "one_stride_differs": "mixed_aligned", "one_shifted": "shifted"}[variant]
    geos = [_geo("mixed_aligned", V), _geo(odd, V), _geo("mixed_aligned", V)]
    imgs = [geos[0].image("out"), geos[1].image("in" if variant == "one_stride_differs" else "out"), geos[2].image("out")]
    if variant == "one_stride_differs":                            # (an `in` view used as an output: its window is the span all the same)
        geos[1].images[0].window = (pc.GUARD_ROWS + SPAN[0], pc.GUARD_ROWS + SPAN[1], 8, 8 + V)
        assert imgs[1].stride(0) != imgs[0].stride(0)
    m = (mod.PulseOsc if kind == "pulse" else mod.TriSawOsc)(V, ctx)
    fr, col = geos[0].per_voice(freq), geos[0].per_voice(color)
    m.paint_batch(zang.Span(*SPAN), imgs, m.Params(SR, zang.constant(fr), col), zero_first=True)
    ctx.sync()
    for b in range(3):
        util.assert_bitexact(util.from_image(imgs[b])[:, SPAN[0]:SPAN[1]], ref[b][:, SPAN[0]:SPAN[1]], f"{kind} batch buffer {b} [{variant}]")
        geos[b].check_canaries(f"{kind} batch buffer {b}")
    assert [int(x) for x in m.state()["cnt"]] == rcnt


# ------------------------------------------------------------------------------------------------ a script module
_SCRIPTS = {}


def _script_program(ctx):
    from zang_amd import script
    if "prog" not in _SCRIPTS:
        text = open(os.path.join(ROOT, "tests", "golden", "script_modules.txt")).read()
        _SCRIPTS["prog"] = script.ScriptProgram(text, ctx, only=["Doubler", "Crush"])
    return _SCRIPTS["prog"]


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("geometry", SMALL_GEOMETRIES)
def test_script_modules_on_views(ctx, geometry, V):
    """Doubler (the first module of tests/golden/script_modules.txt with a buffer parameter) and Crush (a stateful one: Decimator
    into Distortion), output and buffer parameter from different roles, two carried paints against oracle/zs_interp.py"""
    import torch
    from oracle import zangscript as zs, zs_interp
    from zang_amd import zang
    prog = _script_program(ctx)
    compiled = zs.compile(prog.text, prog.filename)
    g = _geo(geometry, V)
    s, e = SPAN
    rng = np.random.default_rng(V + 1)
    x = rng.uniform(-1, 1, (V, FRAMES)).astype(np.float32)
    rate = rng.uniform(-100, 60000, V).astype(np.float32); drive = rng.uniform(0, 1, V).astype(np.float32)
    gx = g.image("in", content=torch.from_numpy(np.ascontiguousarray(x.T)).cuda())
    grate, gdrive = g.per_voice(rate), g.per_voice(drive)
    for name, dev, host in (("Doubler", {"sample_rate": SR, "freq": gx}, lambda v: {"sample_rate": np.float32(SR), "freq": x[v]}),
                            ("Crush", {"sample_rate": SR, "input": gx, "rate": grate, "drive": gdrive},
                             lambda v: {"sample_rate": np.float32(SR), "input": x[v], "rate": np.float32(rate[v]), "drive": np.float32(drive[v])})):
        m = prog.module(name, V, 0)
        voices = zs_interp.make_voices(compiled, name, V, 0)
        order = [p[0] for p in m.params]
        out = g.image("out")
        ref = np.zeros((V, FRAMES), np.float32)
        for k in range(2):
            m.paint(zang.Span(s, e), [out], None, k == 0, dev, zero_first=(k == 0))
            for v in range(V):
                hv = host(v)
                voices[v].paint(s, e, ref[v], k == 0, [hv[n] for n in order])
        ctx.sync()
        util.assert_bitexact(util.from_image(out)[:, s:e], ref[:, s:e], f"{name} [{geometry}]")
        g.check_canaries(name)
        g.release([out])
        m.close()


# ------------------------------------------------------------------------------------------------ validation
def _bad_views(t, V):
    """the three views every entry point must refuse for n = V voices and a span that ends at FRAMES: (what, zh_buf)"""
    from zang_amd import abi
    ptr, stride = t.data_ptr(), t.stride(0)
    return [("voices < n", abi.Buf(ptr, V - 1, FRAMES, stride, 0)), ("frames < span_end", abi.Buf(ptr, V, FRAMES - 1, stride, 0)),
            ("stride < voices", abi.Buf(ptr, V, FRAMES, V - 1, 0))]


def test_views_that_do_not_cover_the_paint_are_refused_without_a_launch(ctx):
    """one paint of each source file (osc.hip, modules.hip, composite.hip, delay.hip, basics.hip, script.hip): a view with voices < n,
    with frames < span_end, with stride < voices is ZH_ERR_INVALID, as the output and as the input / control image; nothing launches"""
    from zang_amd import abi, modules as mod, zang
    V = 68
    g = _geo("shifted", V)
    good, inp = g.image("out", fill=0.0), g.image("in", fill=0.25)
    span = zang.Span(0, FRAMES)
    gc = g.per_voice(np.full(V, 0.5, np.float32))
    pulse, flt, nice, dly = mod.PulseOsc(V, ctx), mod.Filter(V, ctx), mod.NiceInstrument(V, gc, ctx), mod.SimpleDelay(V, DELAY, ctx)
    sm = _script_program(ctx).module("Doubler", V, 0)
    zang.zero(zang.Span(0, 1), good, ctx=ctx)                   # the last launch before the refused calls
    ctx.sync()
    marker = ctx.last_form()
    assert marker == ["k_elementwise"]
    g.images[0].snapshot()
    calls = {
        "osc.hip out": lambda b: pulse.paint(span, [b], [], False, pulse.Params(SR, zang.constant(gc), gc), zero_first=True),
        "osc.hip freq image": lambda b: pulse.paint(span, [good], [], False, pulse.Params(SR, zang.buffer(b), gc), zero_first=True),
        "modules.hip out": lambda b: flt.paint(span, [b], [], False, flt.Params(inp, 1, zang.constant(gc), zang.constant(0.4))),
        "modules.hip input": lambda b: flt.paint(span, [good], [], False, flt.Params(b, 1, zang.constant(gc), zang.constant(0.4))),
        "modules.hip cutoff image": lambda b: flt.paint(span, [good], [], False, flt.Params(inp, 1, zang.buffer(b), zang.constant(0.4))),
        "composite.hip out": lambda b: nice.paint(span, [b], None, True, nice.Params(SR, gc, True)),
        "delay.hip out": lambda b: dly.paint(span, [b], [], False, dly.Params(inp)),
        "delay.hip input": lambda b: dly.paint(span, [good], [], False, dly.Params(b)),
        "basics.hip src": lambda b: zang.copy(span, good, b, ctx=ctx),
        "script.hip out": lambda b: sm.paint(span, [b], None, False, {"sample_rate": SR, "freq": inp}),
    }
    for where, call in calls.items():
        for what, bad in _bad_views(good if where.endswith("out") else inp, V):
            with pytest.raises(abi.ZangHipError, match=r"failed: -1 "):
                call(bad)
            assert ctx.last_form() == marker, (where, what)
    for what, bad in _bad_views(good, V)[1:]:                   # (a destination of fewer voices is a smaller operation, not an error)
        with pytest.raises(abi.ZangHipError, match=r"failed: -1 "):
            zang.copy(span, bad, inp, ctx=ctx)
    with pytest.raises(abi.ZangHipError, match=r"failed: -1 "):  # a script's buffer parameter carries its stride alone
        sm.paint(span, [good], None, False, {"sample_rate": SR, "freq": zang.buffer(_bad_views(inp, V)[2][1])})
    assert ctx.last_form() == marker
    ctx.sync()
    g.check_canaries("refused paints")
    sm.close()
