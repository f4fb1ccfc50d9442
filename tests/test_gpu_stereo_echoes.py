"""GPU parity: StereoEchoes(MAIN_DELAY) (examples/modules.zig:464-525) as one kernel, zh_stereo_echoes_* (csrc/delay.hip).

The oracle is the per-voice composition the reference writes: zo_add_into x2, zo_zero + zo_simple_delay_paint (HALF), zo_zero +
zo_filtered_echoes_paint (MAIN), zo_add_into, zo_simple_delay_paint (HALF) -- in the reference's chunked read-then-write form.  Every
comparison is bit for bit: L, R, the three rings, the three ring indices and the filter's (l, b)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu
F = 1024
SPANS = [(0, 200), (200, 777), (777, 1024), (0, 1024), (0, 1024)]


def _scatter_zeros(a, seed):
    """some -0.0 and +0.0 samples: the `0 +` terms of the composition turn a stored -0.0 into +0.0"""
    rng = np.random.default_rng(seed)
    flat = a.reshape(-1)
    k = max(4, flat.size // 50)
    flat[rng.choice(flat.size, k, replace=False)] = np.float32(-0.0)
    flat[rng.choice(flat.size, k, replace=False)] = np.float32(0.0)
    return a


def _oracle_paints(oracle, V, MAIN, spans, inps, L0, R0, fb, cutoff, zero_first, fresh_outputs=True, state0=None):
    """The composition, voice by voice.  inps[k] / spans[k]: paint k.  fresh_outputs: every paint starts from (L0, R0) again,
    otherwise the paints accumulate into one pair.  state0 = (r0, i0, r1, i1, re, ie) or None (init()).
    Returns (Ls, Rs, (r0, i0, r1, i1, re, ie), l, b) with Ls / Rs one array per paint (or one in all)."""
    L = oracle.lib()
    HALF = MAIN // 2
    frames = L0.shape[1]
    n_out = len(spans) if fresh_outputs else 1
    Ls = [L0.copy() for _ in range(n_out)]; Rs = [R0.copy() for _ in range(n_out)]
    r0 = np.zeros((V, HALF), np.float32); r1 = np.zeros((V, HALF), np.float32); re = np.zeros((V, MAIN), np.float32)
    i0 = np.zeros(V, np.uint32); i1 = np.zeros(V, np.uint32); ie = np.zeros(V, np.uint32)
    fl_l = np.zeros(V, np.float32); fl_b = np.zeros(V, np.float32)
    t0, t1, t2, t3 = (np.zeros(frames, np.float32) for _ in range(4))
    fbv = np.broadcast_to(np.asarray(fb, np.float32), (V,)); cuv = np.broadcast_to(np.asarray(cutoff, np.float32), (V,))
    for v in range(V):
        d0 = oracle.Delay(); L.zo_delay_init(C.byref(d0), oracle.fptr(r0[v]), HALF)
        d1 = oracle.Delay(); L.zo_delay_init(C.byref(d1), oracle.fptr(r1[v]), HALF)
        de = oracle.Delay(); L.zo_delay_init(C.byref(de), oracle.fptr(re[v]), MAIN)
        if state0 is not None:
            r0[v] = state0[0][v]; d0.index = int(state0[1][v])
            r1[v] = state0[2][v]; d1.index = int(state0[3][v])
            re[v] = state0[4][v]; de.index = int(state0[5][v])
        fl = oracle.Filter(); L.zo_filter_init(C.byref(fl))
        for k, (s, e) in enumerate(spans):
            oL = Ls[k if fresh_outputs else 0][v]; oR = Rs[k if fresh_outputs else 0][v]
            x = inps[k][v]
            if zero_first:
                oL[s:e] = 0.0; oR[s:e] = 0.0
            L.zo_add_into(s, e, oracle.fptr(oL), oracle.fptr(x)); L.zo_add_into(s, e, oracle.fptr(oR), oracle.fptr(x))          # :503-504
            L.zo_zero(s, e, oracle.fptr(t0)); L.zo_simple_delay_paint(C.byref(d0), s, e, oracle.fptr(t0), oracle.fptr(x))          # :507-510
            L.zo_zero(s, e, oracle.fptr(t1))                                                                                       # :512
            L.zo_filtered_echoes_paint(C.byref(de), C.byref(fl), s, e, oracle.fptr(t1), oracle.fptr(t2), oracle.fptr(t3), oracle.fptr(t0),
                                       float(fbv[v]), float(cuv[v]))                                                               # :513-517
            L.zo_add_into(s, e, oracle.fptr(oL), oracle.fptr(t1))                                                                  # :519
            L.zo_simple_delay_paint(C.byref(d1), s, e, oracle.fptr(oR), oracle.fptr(t1))                                           # :520-522
        i0[v], i1[v], ie[v] = d0.index, d1.index, de.index
        fl_l[v], fl_b[v] = fl.l, fl.b
    return Ls, Rs, (r0, i0, r1, i1, re, ie), fl_l, fl_b


def _assert_state(m, rings, fl_l, fl_b, what):
    g0, gi0, g1, gi1, ge, gie, gflt = m.state()
    for name, got, ref in (("ring0", g0, rings[0]), ("ring1", g1, rings[2]), ("ring_e", ge, rings[4])):
        util.assert_bitexact(got, ref, f"{what}: {name}")
    for name, got, ref in (("index0", gi0, rings[1]), ("index1", gi1, rings[3]), ("index_e", gie, rings[5])):
        assert np.array_equal(got, ref), f"{what}: {name}"
    util.assert_bitexact(gflt["l"].astype(np.float32), fl_l, f"{what}: l")
    util.assert_bitexact(gflt["b"].astype(np.float32), fl_b, f"{what}: b")


# ------------------------------------------------------------------------------------------------ the main test
V_MAIN = 96


@functools.lru_cache(maxsize=None)
def _main_inputs():
    rng = np.random.default_rng(77)
    fb = rng.uniform(0.1, 0.9, V_MAIN).astype(np.float32); cutoff = rng.uniform(0.05, 1.0, V_MAIN).astype(np.float32)
    inps = [_scatter_zeros(util.rng_buffers(50 + k, V_MAIN, F), 60 + k) for k in range(len(SPANS))]
    return fb, cutoff, inps, util.rng_buffers(7, V_MAIN, F), util.rng_buffers(8, V_MAIN, F)


_main_cache = {}


def _main_reference(oracle, MAIN, zero_first):
    """one oracle run per (MAIN, zero_first), shared by the forms and never written to"""
    key = (MAIN, zero_first)
    if key not in _main_cache:
        fb, cutoff, inps, L0, R0 = _main_inputs()
        _main_cache[key] = _oracle_paints(oracle, V_MAIN, MAIN, SPANS, inps, L0, R0, fb, cutoff, zero_first)
    return _main_cache[key]


def _run_main(ctx, oracle, MAIN, zero_first):
    from zang_amd import modules as mod, zang
    fb, cutoff, inps, L0, R0 = _main_inputs()
    refL, refR, rings, fl_l, fl_b = _main_reference(oracle, MAIN, zero_first)
    m = mod.StereoEchoes(V_MAIN, MAIN, ctx)
    gfb, gc = util.dev(fb), util.dev(cutoff)
    for k, (s, e) in enumerate(SPANS):
        gl, gr = util.to_image(L0), util.to_image(R0)
        m.paint(zang.Span(s, e), [gl, gr], None, False, m.Params(util.to_image(inps[k]), gfb, gc), zero_first=zero_first)
        ctx.sync()
        util.assert_bitexact(util.from_image(gl), refL[k], f"stereo echoes MAIN={MAIN} paint {k} L")
        util.assert_bitexact(util.from_image(gr), refR[k], f"stereo echoes MAIN={MAIN} paint {k} R")
    _assert_state(m, rings, fl_l, fl_b, f"MAIN={MAIN}")
    m.reset()                                                  # :488-492: the three delays; the filter keeps (l, b)
    g0, gi0, g1, gi1, ge, gie, gflt = m.state()
    assert not g0.any() and not g1.any() and not ge.any() and not gi0.any() and not gi1.any() and not gie.any()
    util.assert_bitexact(gflt["l"].astype(np.float32), fl_l, "l after reset")
    util.assert_bitexact(gflt["b"].astype(np.float32), fl_b, "b after reset")
    m.close()


@pytest.mark.parametrize("form", ["default", "walk"])
@pytest.mark.parametrize("zero_first", [False, True])
@pytest.mark.parametrize("MAIN", [2, 3, 15, 16, 17, 191, 192, 385, 400, 1024, 2048, 2500])
def test_stereo_echoes(ctx, oracle, MAIN, zero_first, form, monkeypatch):
    """HALF = 1, 1, 7, 8, 8 either side of the 8-frame chunking; 191 / 192 / 385 / 400 either side of the role waves' minimum; HALF =
    512 (half of the 1,024-frame paint), 1,024 (the whole paint) and 1,250 (longer than any paint).  `walk`: stereo_echoes_pc_max = 0."""
    if form == "walk":
        util.set_form(monkeypatch, stereo_echoes_pc_max="0")
    _run_main(ctx, oracle, MAIN, zero_first)


def test_stereo_echoes_15000(ctx, oracle):
    """the reference's own use: StereoEchoes(15000) (example_delay.zig:69-79), zero-first"""
    _run_main(ctx, oracle, 15000, True)


# ------------------------------------------------------------------------------------------------ broadcast scalars; the device composition
def test_stereo_echoes_broadcast_scalars_equal_oracle_and_device_composition(ctx, oracle):
    from zang_amd import modules as mod, zang
    V, MAIN = 96, 1500
    HALF = MAIN // 2
    inps = [_scatter_zeros(util.rng_buffers(130 + k, V, F), 140 + k) for k in range(3)]
    L0, R0 = util.rng_buffers(17, V, F), util.rng_buffers(18, V, F)
    spans = [(0, F)] * 3
    refL, refR, rings, fl_l, fl_b = _oracle_paints(oracle, V, MAIN, spans, inps, L0, R0, 0.6, 0.1, False)
    m = mod.StereoEchoes(V, MAIN, ctx)
    delay0, delay1, echoes = mod.SimpleDelay(V, HALF, ctx), mod.SimpleDelay(V, HALF, ctx), mod.FilteredEchoes(V, MAIN, ctx)
    sp = zang.Span(0, F)
    g0, g1 = ctx.image(F, V), ctx.image(F, V)
    for k in range(3):
        gin = util.to_image(inps[k])
        gl, gr = util.to_image(L0), util.to_image(R0)
        m.paint(sp, [gl, gr], None, False, m.Params(gin, 0.6, 0.1))
        cl, cr = util.to_image(L0), util.to_image(R0)
        zang.addInto(sp, cl, gin, ctx=ctx); zang.addInto(sp, cr, gin, ctx=ctx)
        delay0.paint(sp, [g0], [], False, delay0.Params(gin), zero_first=True)
        echoes.paint(sp, [g1], None, False, echoes.Params(g0, 0.6, 0.1), zero_first=True)
        zang.addInto(sp, cl, g1, ctx=ctx)
        delay1.paint(sp, [cr], [], False, delay1.Params(g1))
        ctx.sync()
        util.assert_bitexact(util.from_image(gl), refL[k], f"L {k} vs oracle"); util.assert_bitexact(util.from_image(gr), refR[k], f"R {k} vs oracle")
        util.assert_bitexact(util.from_image(gl), util.from_image(cl), f"L {k} vs device composition")
        util.assert_bitexact(util.from_image(gr), util.from_image(cr), f"R {k} vs device composition")
    _assert_state(m, rings, fl_l, fl_b, "broadcast scalars")
    util.assert_bitexact(m.state()[0], delay0.state()[0], "ring0 vs SimpleDelay")
    util.assert_bitexact(m.state()[2], delay1.state()[0], "ring1 vs SimpleDelay")
    util.assert_bitexact(m.state()[4], echoes.state()[0], "ring_e vs FilteredEchoes")


# ------------------------------------------------------------------------------------------------ per-voice ring indices (set_state)
@pytest.mark.parametrize("form", ["default", "walk"])
@pytest.mark.parametrize("MAIN", [400, 667])
def test_stereo_echoes_per_voice_ring_indices(ctx, oracle, MAIN, form, monkeypatch):
    """set_state gives every voice its own three ring indices and ring contents: the role waves take their per-lane slot
    arithmetic (no wave-uniform row addressing), each ring wrapping at a different frame per voice."""
    from zang_amd import abi, modules as mod, zang
    if form == "walk":
        util.set_form(monkeypatch, stereo_echoes_pc_max="0")
    V, HALF = 130, MAIN // 2
    rng = np.random.default_rng(91)
    state0 = (rng.uniform(-1, 1, (V, HALF)).astype(np.float32), rng.integers(0, HALF, V).astype(np.uint32),
              rng.uniform(-1, 1, (V, HALF)).astype(np.float32), rng.integers(0, HALF, V).astype(np.uint32),
              rng.uniform(-1, 1, (V, MAIN)).astype(np.float32), rng.integers(0, MAIN, V).astype(np.uint32))
    fb = rng.uniform(0.1, 0.9, V).astype(np.float32); cutoff = rng.uniform(0.05, 1.0, V).astype(np.float32)
    inp = _scatter_zeros(util.rng_buffers(92, V, F), 93)
    L0, R0 = util.rng_buffers(94, V, F), util.rng_buffers(95, V, F)
    spans = [(0, 1024), (100, 612), (612, 1000)]
    refL, refR, rings, fl_l, fl_b = _oracle_paints(oracle, V, MAIN, spans, [inp] * 3, L0, R0, fb, cutoff, False, fresh_outputs=False, state0=state0)
    m = mod.StereoEchoes(V, MAIN, ctx)
    m.set_state(*state0, np.zeros(V, dtype=np.dtype(abi.FilterState)))
    gl, gr, gin = util.to_image(L0), util.to_image(R0), util.to_image(inp)
    gfb, gc = util.dev(fb), util.dev(cutoff)
    for (s, e) in spans:
        m.paint(zang.Span(s, e), [gl, gr], None, False, m.Params(gin, gfb, gc))
    ctx.sync()
    util.assert_bitexact(util.from_image(gl), refL[0], "L, per-voice indices"); util.assert_bitexact(util.from_image(gr), refR[0], "R, per-voice indices")
    _assert_state(m, rings, fl_l, fl_b, "per-voice indices")
    bad = list(state0) + [np.zeros(V, dtype=np.dtype(abi.FilterState))]
    for which, limit in ((1, HALF), (3, HALF), (5, MAIN)):     # an index that is not below its ring's length
        idx = bad[which].copy(); idx[V // 2] = limit
        args = bad[:which] + [idx] + bad[which + 1:]
        with pytest.raises(abi.ZangHipError):
            m.set_state(*args)
    _assert_state(m, rings, fl_l, fl_b, "after refused set_state")


# ------------------------------------------------------------------------------------------------ views
NAN_BITS = 0x7FC00ABC


def _nan_backing(rows, cols):
    import torch
    return torch.full((rows, cols), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


@pytest.mark.parametrize("MAIN", [100, 400])
@pytest.mark.parametrize("geometry", ["separate", "one_allocation"])
@pytest.mark.parametrize("V", [68, 256])
def test_stereo_echoes_on_views(ctx, oracle, V, geometry, MAIN):
    """Input, L and R are views of NaN-filled allocations: row strides that are no multiple of 4 floats (V + 7; 3 V + 15 for the three
    column ranges of one allocation), bases one float past a 16-byte boundary.  The result equals the oracle and no element outside
    the views' span rows changes.  MAIN = 100: the walk; 400: the role waves (321 frames: ten tiles and a partial one)."""
    import torch
    from zang_amd import modules as mod, zang
    FR, (s, e), G = 352, (13, 334), 4
    rng = np.random.default_rng(5)
    fb = rng.uniform(0.1, 0.9, V).astype(np.float32); cutoff = rng.uniform(0.05, 1.0, V).astype(np.float32)
    inp = _scatter_zeros(util.rng_buffers(101, V, FR), 102)
    L0, R0 = util.rng_buffers(103, V, FR), util.rng_buffers(104, V, FR)
    (refL,), (refR,), rings, fl_l, fl_b = _oracle_paints(oracle, V, MAIN, [(s, e)], [inp], L0, R0, fb, cutoff, False)
    if geometry == "separate":
        backs = [_nan_backing(FR + 2 * G, V + 7) for _ in range(3)]
        views = [b[G:G + FR, 1:1 + V] for b in backs]
    else:
        back = _nan_backing(FR + 2 * G, 3 * V + 15)
        backs = [back]
        views = [back[G:G + FR, c:c + V] for c in (1, V + 5, 2 * V + 9)]
    for view in views:
        assert view.stride(0) % 4 != 0 and (view.data_ptr() // 4) % 4 == 1
    vin, vl, vr = views
    vin.copy_(util.to_image(inp)); vl.copy_(util.to_image(L0)); vr.copy_(util.to_image(R0))
    before = [b.clone() for b in backs]
    m = mod.StereoEchoes(V, MAIN, ctx)
    m.paint(zang.Span(s, e), [vl, vr], None, False, m.Params(vin, util.dev(fb), util.dev(cutoff)))
    ctx.sync()
    util.assert_bitexact(util.from_image(vl), refL, f"L on views ({geometry})"); util.assert_bitexact(util.from_image(vr), refR, f"R on views ({geometry})")
    _assert_state(m, rings, fl_l, fl_b, "views")
    # everything but the span rows of the two output views is as it was (the input view included)
    vl[s:e].copy_(util.to_image(L0)[s:e]); vr[s:e].copy_(util.to_image(R0)[s:e])
    for b, b0 in zip(backs, before):
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32)), "an element outside the painted rows changed"


@pytest.mark.parametrize("MAIN", [100, 400])
def test_stereo_echoes_on_touching_column_ranges(ctx, oracle, MAIN):
    """The three images as the column ranges [0, V), [V, 2 V), [2 V, 3 V) of one allocation of stride 3 V: they share no float although
    their extents interleave, and the last one ends exactly where the next row begins (the accepting edge of the overlap test).  The
    result equals the oracle.  Moved one column to the left, the right output shares a column with the left one: refused, no launch."""
    import torch
    from zang_amd import abi, modules as mod, zang
    V, FR, (s, e) = 68, 352, (13, 334)
    rng = np.random.default_rng(6)
    fb = rng.uniform(0.1, 0.9, V).astype(np.float32); cutoff = rng.uniform(0.05, 1.0, V).astype(np.float32)
    inp = _scatter_zeros(util.rng_buffers(121, V, FR), 122)
    L0, R0 = util.rng_buffers(123, V, FR), util.rng_buffers(124, V, FR)
    (refL,), (refR,), rings, fl_l, fl_b = _oracle_paints(oracle, V, MAIN, [(s, e)], [inp], L0, R0, fb, cutoff, False)
    back = torch.zeros((FR, 3 * V), dtype=torch.float32, device="cuda")
    vin, vl, vr = back[:, :V], back[:, V:2 * V], back[:, 2 * V:]
    vin.copy_(util.to_image(inp)); vl.copy_(util.to_image(L0)); vr.copy_(util.to_image(R0))
    m = mod.StereoEchoes(V, MAIN, ctx)
    P = m.Params(vin, util.dev(fb), util.dev(cutoff))
    zang.zero(zang.Span(0, 1), ctx.image(1, V), ctx=ctx)
    marker = ctx.last_form()
    for bad in ([vl, back[:, 2 * V - 1:3 * V - 1]], [back[:, V - 1:2 * V - 1], vr]):       # R over L's last column; L over the input's
        with pytest.raises(abi.ZangHipError, match=r"failed: -1 "):
            m.paint(zang.Span(s, e), bad, None, False, P)
        assert ctx.last_form() == marker, ctx.last_form()
    m.paint(zang.Span(s, e), [vl, vr], None, False, P)
    ctx.sync()
    util.assert_bitexact(util.from_image(vl), refL, "L, touching columns"); util.assert_bitexact(util.from_image(vr), refR, "R, touching columns")
    util.assert_bitexact(util.from_image(vin), inp, "the input is untouched")
    _assert_state(m, rings, fl_l, fl_b, "touching columns")


# ------------------------------------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("MAIN", [100, 400])
def test_stereo_echoes_in_a_graph(MAIN):
    """a paint neither allocates nor synchronises: recorded in a graph and replayed twice, it equals two direct paints"""
    import torch
    from zang_amd import modules as mod, zang
    import zang_amd
    V = 96
    inp = util.rng_buffers(111, V, F); L0, R0 = util.rng_buffers(112, V, F), util.rng_buffers(113, V, F)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        md, mg = mod.StereoEchoes(V, MAIN, c2), mod.StereoEchoes(V, MAIN, c2)
        gin = util.to_image(inp)
        dl, dr, gl, gr = util.to_image(L0), util.to_image(R0), util.to_image(L0), util.to_image(R0)
        sp = zang.Span(0, F)
        md.paint(sp, [dl, dr], None, False, md.Params(gin, 0.6, 0.1)); md.paint(sp, [dl, dr], None, False, md.Params(gin, 0.6, 0.1))
        c2.sync()
        g = c2.capture(lambda: mg.paint(sp, [gl, gr], None, False, mg.Params(gin, 0.6, 0.1)))
        g.launch(); g.launch()
        c2.sync()
        assert torch.equal(gl.view(torch.int32), dl.view(torch.int32)) and torch.equal(gr.view(torch.int32), dr.view(torch.int32))
        sd, sg = md.state(), mg.state()
        for a, b in zip(sd[:6], sg[:6]):
            util.assert_bitexact(a, b, "state after the replays")
        util.assert_bitexact(sd[6]["l"].astype(np.float32), sg[6]["l"].astype(np.float32), "l")
        util.assert_bitexact(sd[6]["b"].astype(np.float32), sg[6]["b"].astype(np.float32), "b")
        g.close(); c2.close()


# ------------------------------------------------------------------------------------------------ kernel names, refusals
def test_stereo_echoes_kernel_names(ctx):
    from zang_amd import modules as mod, zang
    V = 96
    gin, gl, gr = ctx.image(F, V, fill=0.25), ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)
    marker = ["k_elementwise"]                                 # zh_last_form keeps the last launch: a call that launches nothing leaves it
    for MAIN, name in ((400, "k_stereo_echoes_pc"), (100, "k_stereo_echoes")):
        m = mod.StereoEchoes(V, MAIN, ctx)
        m.paint(zang.Span(0, F), [gl, gr], None, False, m.Params(gin, 0.6, 0.1))
        assert ctx.last_form() == [name], (MAIN, ctx.last_form())
        zang.zero(zang.Span(0, 1), gl, ctx=ctx)
        assert ctx.last_form() == marker
        m.paint(zang.Span(5, 5), [gl, gr], None, False, m.Params(gin, 0.6, 0.1))       # an empty span: ZH_OK, no launch
        assert ctx.last_form() == marker, ctx.last_form()
    m0 = mod.StereoEchoes(0, 400, ctx)                                                 # no voices: ZH_OK, no launch
    m0.paint(zang.Span(0, F), [gl, gr], None, False, m0.Params(gin, 0.6, 0.1))
    assert ctx.last_form() == marker, ctx.last_form()
    ctx.sync()


def test_stereo_echoes_refusals_launch_nothing(ctx):
    import torch
    from zang_amd import abi, modules as mod, zang
    V = 96
    for bad in (0, 1):
        with pytest.raises(abi.ZangHipError):
            mod.StereoEchoes(V, bad, ctx)
    m = mod.StereoEchoes(V, 400, ctx)
    big = torch.full((2 * F, V), 0.5, dtype=torch.float32, device="cuda")
    gin, gl, gr = ctx.image(F, V, fill=0.25), ctx.image(F, V, fill=1.0), ctx.image(F, V, fill=2.0)
    sp, P = zang.Span(0, F), m.Params(gin, 0.6, 0.1)
    state0 = m.state()
    zang.zero(zang.Span(0, 1), big, ctx=ctx)                   # the last launch before the refused calls: zh_last_form keeps naming it
    marker = ctx.last_form()
    assert marker == ["k_elementwise"]

    def refused(code, fn):
        with pytest.raises(abi.ZangHipError) as ei:
            fn()
        assert f"failed: {code} (" in str(ei.value), ei.value
        assert ctx.last_form() == marker, ctx.last_form()

    refused(abi.ZH_ERR_INVALID, lambda: m.paint(sp, [gl, gl], None, False, P))                                      # L is R
    refused(abi.ZH_ERR_INVALID, lambda: m.paint(sp, [gin, gr], None, False, P))                                     # the input is L
    refused(abi.ZH_ERR_INVALID, lambda: m.paint(sp, [big[F - 1:2 * F - 1], gr], None, False, m.Params(big[:F], 0.6, 0.1)))   # one shared row
    refused(abi.ZH_ERR_INVALID, lambda: m.paint(sp, [gl, gr[:F - 1]], None, False, P))                               # one frame too short
    refused(abi.ZH_ERR_INVALID, lambda: m.paint(sp, [gl, gr], None, False, m.Params(gin[:F - 1], 0.6, 0.1)))
    refused(abi.ZH_ERR_INVALID, lambda: m.paint(zang.Span(9, 3), [gl, gr], None, False, P))                         # end < start
    refused(abi.ZH_ERR_UNSUPPORTED, lambda: m.paint(sp, [gl, gr], None, False, P, tolerant=True))
    ctx.sync()
    assert float(gl.min()) == 1.0 == float(gl.max()) and float(gr.min()) == 2.0 == float(gr.max())
    for a, b in zip(state0[:6], m.state()[:6]):
        util.assert_bitexact(a, b, "state after refusals")
