"""GPU: every voice mixdown against tests/mix_order_reference.py, the numpy float32 restatement of its documented summation order, bit
for bit in every frame -- zh_mixdown_voices in its tree form (k_mix_pass1 / k_mix_pass1_scalar + k_mix_pass2) and the fused
NiceInstrument mixdowns zh_nice_paint_mix / _stereo / _stereo_batch (k_nice_mix / k_nice_mix_batch + k_mix_pass2_wide).

Destinations are pre-filled with random values and compared whole, guard elements included: what lies outside the span keeps its bits.
Both zero_first values run, and the kernels that ran are asserted (zh_last_form).  The fused model's input is the per-voice image of a
twin NiceInstrument painted with the same script (tests/test_gpu_composite.py holds that paint to the oracle bit for bit); the twin's
final state must equal every mixing module's."""
import os

import numpy as np
import pytest

from tests import mix_order_cases as mc
from tests import mix_order_reference as mo
from tests import paint_cases as pc
from tests import util

pytestmark = pytest.mark.gpu
SR = 48000.0
F32 = np.float32
GUARD = 4                      # floats before and after a destination row


def _clear_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("ZH_") and name not in ("ZH_ENV_LIVE",):
            monkeypatch.delenv(name)                           # default dispatch, whatever the suite was started with


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------------------------------------ zh_mixdown_voices
class _Source:
    """src [V][rows] on the device in one of two layouts.  `aligned`: every row 16-byte aligned (row stride a multiple of four floats)
    whatever V is -- k_mix_pass1 and its float4 loads; `view`: a paint_cases geometry with an odd stride, or, where V + 11 is a
    multiple of four, a base 4 mod 16 -- k_mix_pass1_scalar.  Canaries around both."""

    def __init__(self, src, layout):
        torch = _torch()
        V, rows = src.shape
        content = torch.from_numpy(np.ascontiguousarray(src.T)).cuda()
        self.layout = layout
        if layout == "aligned":
            stride = (V + 3) // 4 * 4 + 4
            self.backing = torch.full((rows + 2, stride), pc.CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
            self.img = self.backing[1:1 + rows, :V]
            self.img.copy_(content)
            self.snap = self.backing.view(torch.int32).clone()
            assert self.img.data_ptr() % 16 == 0 and self.img.stride(0) % 4 == 0
            self.kernel = "k_mix_pass1"
        else:
            name = "odd_stride" if (V + 11) % 4 else "shifted"
            self.geo = pc.Geometry(name, V, frames=rows)
            self.img = self.geo.image("in", content=content)
            assert self.img.stride(0) % 4 or self.img.data_ptr() % 16 == 4, name
            self.kernel = "k_mix_pass1_scalar"

    def check(self, what):
        if self.layout == "aligned":
            assert bool((self.backing.view(_torch().int32) == self.snap).all()), what
        else:
            self.geo.check_canaries(what)


def _tree_run(ctx, source, src, span, zero_first, dst_row, offset):
    """one zh_mixdown_voices call into dst_row (host, with guards) at `offset`; returns (got, want) as whole rows"""
    from zang_amd import zang
    rows = src.shape[1]
    full = util.dev(dst_row)
    mix = full[offset:offset + rows]
    zang.mixdownVoices(zang.Span(*span), mix, source.img, zero_first=zero_first, ctx=ctx)
    form = ctx.last_form()
    ctx.sync()
    want = dst_row.copy()
    want[offset:offset + rows] = mo.tree_mix_span(src, dst_row[offset:offset + rows], span[0], span[1], zero_first)
    return full.cpu().numpy(), want, form


@pytest.mark.parametrize("layout", ["aligned", "view"])
@pytest.mark.parametrize("V", mc.TREE_VS)
def test_mixdown_voices_is_the_tree_order(ctx, V, layout, monkeypatch):
    """Quad tails, wave and tile edges, one to 34 tiles, spans under, at and over the first pass's 8-frame group and the second
    pass's 64-frame block, onto a random destination and with zero_first: the model's bits in every frame."""
    _clear_env(monkeypatch)
    src = mc.random_image(V, mc.TREE_ROWS)
    source = _Source(src, layout)
    offset = GUARD if layout == "aligned" else 1
    for k, span in enumerate(mc.TREE_SPANS):
        for zero_first in (False, True):
            dst_row = mc.random_row(mc.TREE_ROWS + 2 * GUARD, 100 * k + zero_first)
            got, want, form = _tree_run(ctx, source, src, span, zero_first, dst_row, offset)
            if span[1] > span[0]:
                assert form == [source.kernel, "k_mix_pass2"], (span, form)
            util.assert_bitexact(got, want, f"tree mixdown V={V} {layout} span={span} zero_first={zero_first}")
    source.check(f"tree mixdown V={V}")


@pytest.mark.parametrize("layout", ["aligned", "view"])
@pytest.mark.parametrize("V", mc.PLANTED_VS)
def test_mixdown_voices_planted_columns(ctx, V, layout, monkeypatch):
    """The cancellation columns (their sums derived by hand in tests/mix_order_cases.py: 0.0 or 1.0 according to where 1e8, 1.0 and -1e8
    sit), an all -0.0 image (+0.0, onto -0.0 as well), subnormal voices (summed, not flushed), and one NaN, one +Inf and one -Inf:
    those three frames are compared by class, every other frame by bits."""
    _clear_env(monkeypatch)
    # -- cancellation
    img, want_hand = mc.planted_image(V)
    n = img.shape[1]
    source = _Source(img, layout)
    for zero_first in (True, False):
        dst_row = mc.random_row(n + 2 * GUARD, 11 + zero_first)
        got, want, form = _tree_run(ctx, source, img, (0, n), zero_first, dst_row, GUARD)
        assert form == [source.kernel, "k_mix_pass2"], form
        util.assert_bitexact(got, want, f"planted columns V={V} zero_first={zero_first}")
        if zero_first:
            util.assert_bitexact(got[GUARD:GUARD + n], want_hand, f"planted columns V={V} against the hand-derived sums")
    source.check("planted columns")
    # -- signed zeros
    neg = np.full((V, 16), -0.0, F32)
    source = _Source(neg, layout)
    for zero_first in (True, False):
        dst_row = mc.random_row(16 + 2 * GUARD, 21)
        dst_row[GUARD:GUARD + 8] = -0.0
        got, want, _ = _tree_run(ctx, source, neg, (0, 16), zero_first, dst_row, GUARD)
        util.assert_bitexact(got, want, f"-0.0 image V={V} zero_first={zero_first}")
        assert (got[GUARD:GUARD + 8].view(np.uint32) == 0).all()                      # +0.0, whatever zero_first
    # -- subnormals and non-finite voices
    img, classes = mc.special_image(V)
    assert len(classes) <= 3
    n = img.shape[1]
    source = _Source(img, layout)
    by_bits = np.array([f not in classes for f in range(n)])
    for zero_first in (True, False):
        dst_row = mc.random_row(n + 2 * GUARD, 31 + zero_first)
        got, want, _ = _tree_run(ctx, source, img, (0, n), zero_first, dst_row, GUARD)
        keep = np.ones(len(got), bool)
        keep[GUARD:GUARD + n] = by_bits
        util.assert_bitexact(got[keep], want[keep], f"special voices V={V} zero_first={zero_first}")
        for f, cls in classes.items():
            assert mc.float_class(got[GUARD + f]) == cls == mc.float_class(want[GUARD + f]), (f, cls, got[GUARD + f])
        if zero_first:
            assert got[GUARD + 2] > 0.0 and got[GUARD + 2] == want[GUARD + 2]          # V subnormal voices: not flushed
    source.check("special voices")


# ------------------------------------------------------------------------------------------------ the fused NiceInstrument mixdown
# note on with a new id, held, note off (release tails), over the spans of the 128-row image
SCRIPT = [(mc.FUSED_SPANS[0], 1, 1), (mc.FUSED_SPANS[1], 1, 0), (mc.FUSED_SPANS[2], 0, 0), (mc.FUSED_SPANS[3], 0, 0), (mc.FUSED_SPANS[4], 0, 0)]
SCRIPT_TALL = [((0, 1024), 1, 1), ((0, 1024), 1, 0), ((0, 1024), 0, 0)]
MIX_FORM = ["k_nice_mix", "k_mix_pass2_wide"]


def _voices(V):
    from zang_amd import workloads
    freq, color, u2, _ = workloads.voice_params(5, 7, V)
    gl, gr = mc.fused_gains(u2)
    return mc.silence_some(freq), color, gl, gr


def _set_rows(monkeypatch, V, rows_per):
    """default dispatch, or nice_mix_wg_min = 0 (one partial row per workgroup at any voice count); returns the model's row form"""
    _clear_env(monkeypatch)
    if rows_per == "default":
        return mo.rows_per_for(V)
    if rows_per == "workgroup":
        util.set_form(monkeypatch, nice_mix_wg_min=0)
    else:
        assert rows_per == mo.rows_per_for(V) == "wave"
    return rows_per


def _fused_script(ctx, V, rows, script, rows_per):
    """The script on a twin (per-voice paint) and on five mixing modules: mono and stereo, each onto its destination and with
    zero_first, and stereo with both gains 1.0.  Every paint: eight destination rows against the model, whole rows."""
    torch = _torch()
    from zang_amd import modules as mod, zang
    freq, color, gl, gr = _voices(V)
    gc, gf, dgl, dgr = util.dev(color), util.dev(freq), util.dev(gl), util.dev(gr)
    twin, mono0, mono1, st0, st1, unit = (mod.NiceInstrument(V, gc, ctx) for _ in range(6))
    peak = 0.0
    for k, ((s, e), on, nic) in enumerate(script):
        span = zang.Span(s, e)
        P = twin.Params(SR, gf, bool(on))
        per_voice = ctx.image(rows, V, fill=0.0)
        twin.paint(span, [per_voice], None, bool(nic), P)
        start = np.random.default_rng(1000 * V + k).uniform(-1.0, 1.0, (8, rows + 2 * GUARD)).astype(F32)
        wide = util.dev(start)
        d = [wide[i, GUARD:GUARD + rows] for i in range(8)]
        forms = []
        mono0.paint_mix(span, d[0], bool(nic), P); forms.append(ctx.last_form())
        mono1.paint_mix(span, d[1], bool(nic), P, zero_first=True); forms.append(ctx.last_form())
        st0.paint_mix_stereo(span, d[2], d[3], dgl, dgr, bool(nic), P); forms.append(ctx.last_form())
        st1.paint_mix_stereo(span, d[4], d[5], dgl, dgr, bool(nic), P, zero_first=True); forms.append(ctx.last_form())
        unit.paint_mix_stereo(span, d[6], d[7], 1.0, 1.0, bool(nic), P, zero_first=True); forms.append(ctx.last_form())
        ctx.sync()
        for form in forms:                                     # the exact kernels, never the tolerant ones; an empty span has no second pass
            assert form == (MIX_FORM if e > s else MIX_FORM[:1]), (k, form)
        pv = per_voice.cpu().numpy()
        peak = max(peak, float(np.abs(pv[s:e]).max()) if e > s else 0.0)
        h = [start[i, GUARD:GUARD + rows] for i in range(8)]
        want = start.copy()
        w = [want[i, GUARD:GUARD + rows] for i in range(8)]
        w[0][:] = mo.fused_mix_span(pv, None, h[0], s, e, False, rows_per)
        w[1][:] = mo.fused_mix_span(pv, None, h[1], s, e, True, rows_per)
        w[2][:], w[3][:] = mo.fused_mix_span(pv, (gl, gr), (h[2], h[3]), s, e, False, rows_per)
        w[4][:], w[5][:] = mo.fused_mix_span(pv, (gl, gr), (h[4], h[5]), s, e, True, rows_per)
        w[6][:], w[7][:] = mo.fused_mix_span(pv, (1.0, 1.0), (h[6], h[7]), s, e, True, rows_per)
        got = wide.cpu().numpy()
        for i, name in enumerate(["mono +=", "mono zero_first", "left +=", "right +=", "left zero_first", "right zero_first", "unit left", "unit right"]):
            util.assert_bitexact(got[i], want[i], f"fused mixdown V={V} rows per {rows_per}, paint {k} span=({s}, {e}): {name}")
        g = got[:, GUARD + s:GUARD + e]
        util.assert_bitexact(g[6], g[1], "both gains 1.0: left == mono"); util.assert_bitexact(g[7], g[1], "both gains 1.0: right == mono")
    assert peak > 1e-3, peak                                    # the script is audible: the sums are not sums of zeros
    ref = twin.state()
    for name, m in (("mono +=", mono0), ("mono zero_first", mono1), ("stereo +=", st0), ("stereo zero_first", st1), ("unit gains", unit)):
        assert np.array_equal(ref, m.state()), name


@pytest.mark.parametrize("rows_per", ["wave", "workgroup"])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_fused_mixdown_is_the_documented_order(ctx, V, rows_per, monkeypatch):
    """Half-row chains, h0 + h1, dead lanes and dead waves, in both row forms: per-wave rows (the default below 65,536 voices) and one
    row per workgroup (nice_mix_wg_min = 0)."""
    rows_per = _set_rows(monkeypatch, V, rows_per)
    _fused_script(ctx, V, mc.FUSED_ROWS, SCRIPT, rows_per)


@pytest.mark.parametrize("V,rows_per", [(8256, "wave"),            # 129 wave rows: a second-pass thread class with two rows
                                        (33024, "workgroup"),      # 129 workgroup rows (nice_mix_wg_min = 0)
                                        (65792, "default"),        # as shipped: 257 workgroup rows, class 0 adds three
                                        (65600, "default")])       # ... and a last workgroup whose waves 1 .. 3 are dead
def test_fused_mixdown_second_pass_classes(ctx, V, rows_per, monkeypatch):
    rows_per = _set_rows(monkeypatch, V, rows_per)
    assert rows_per == ("wave" if V == 8256 else "workgroup")
    _fused_script(ctx, V, mc.FUSED_ROWS, SCRIPT, rows_per)


def test_fused_mixdown_tall_span(ctx, monkeypatch):
    """(0, 1024) at 1,000 voices: 32 whole chunks, attack to sustain to release"""
    rows_per = _set_rows(monkeypatch, 1000, "default")
    assert rows_per == "wave"
    _fused_script(ctx, 1000, 1024, SCRIPT_TALL, rows_per)


@pytest.mark.parametrize("rows_per", ["wave", "workgroup"])
def test_fused_mixdown_batch_is_the_documented_order(ctx, rows_per, monkeypatch):
    """zh_nice_paint_mix_stereo_batch, three buffers whose freq, note_on and note_id_changed differ, 257 voices, two spans: the model
    buffer by buffer on a twin that paints the three one after the other."""
    from zang_amd import modules as mod, zang
    V, rows = 257, mc.FUSED_ROWS
    rows_per = _set_rows(monkeypatch, V, rows_per)
    freq, color, gl, gr = _voices(V)
    freq_b = mc.silence_some(np.roll(freq, 7) * F32(1.5))
    gc, dgl, dgr = util.dev(color), util.dev(gl), util.dev(gr)
    gfa, gfb = util.dev(freq), util.dev(freq_b)
    twin, b0, b1 = (mod.NiceInstrument(V, gc, ctx) for _ in range(3))
    buffers = [[(gfa, True, True), (gfb, True, False), (gfa, False, False)],
               [(gfb, True, True), (gfb, False, False), (gfa, True, True)]]
    for k, (s, e) in enumerate([(5, 78), (0, 32)]):
        span = zang.Span(s, e)
        Ps = [twin.Params(SR, f, on) for f, on, _ in buffers[k]]
        nics = [nic for _, _, nic in buffers[k]]
        pvs = []
        for P, nic in zip(Ps, nics):
            img = ctx.image(rows, V, fill=0.0)
            twin.paint(span, [img], None, nic, P)
            pvs.append(img)
        start = np.random.default_rng(50 + k).uniform(-1.0, 1.0, (12, rows + 2 * GUARD)).astype(F32)
        wide = util.dev(start)
        d = [wide[i, GUARD:GUARD + rows] for i in range(12)]
        b0.paint_mix_stereo_batch(span, d[0:3], d[3:6], dgl, dgr, nics, Ps)
        form0 = ctx.last_form()
        b1.paint_mix_stereo_batch(span, d[6:9], d[9:12], dgl, dgr, nics, Ps, zero_first=True)
        form1 = ctx.last_form()
        ctx.sync()
        assert form0 == form1 == ["k_nice_mix_batch", "k_mix_pass2_wide"], (form0, form1)
        want = start.copy()
        for b in range(3):
            pv = pvs[b].cpu().numpy()
            assert np.abs(pv[s:e]).max() > 0.0
            for base, zero_first in ((0, False), (6, True)):
                l, r = mo.fused_mix_span(pv, (gl, gr), (start[base + b, GUARD:GUARD + rows], start[base + 3 + b, GUARD:GUARD + rows]), s, e, zero_first, rows_per)
                want[base + b, GUARD:GUARD + rows] = l
                want[base + 3 + b, GUARD:GUARD + rows] = r
        util.assert_bitexact(wide.cpu().numpy(), want, f"batch rows per {rows_per}, span ({s}, {e})")
    assert np.array_equal(twin.state(), b0.state()) and np.array_equal(twin.state(), b1.state())
