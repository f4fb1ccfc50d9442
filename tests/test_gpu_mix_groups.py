"""GPU: the grouped voice mixdown (zh_mixdown_groups / zh_mixdown_groups_pcm, csrc/mix_groups.hip) against a numpy f32 add-by-add
loop, the oracle's mixDown and the composition it replaces (zh_mixdown_voices(ZH_MIX_SEQUENTIAL) per group + zh_mix_down).  No
tolerance: ordered f32 adds, one multiply, an integer conversion -- a NaN equals any NaN (mix_groups_cases.same_f32)."""
import numpy as np
import pytest

from tests import mix_groups_cases as mg
from tests import voice_bank_cases as vb

pytestmark = pytest.mark.gpu
F = 1024
VOL = 0.25
S16, S8 = 1, 0


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _image(ctx, img, pad=0, shift=0):
    """the host image as a device view with `pad` more floats per row, starting `shift` floats into its block"""
    import torch
    frames, V = img.shape
    block = torch.full((frames * (V + pad) + shift,), 777.0, dtype=torch.float32, device=ctx.device)
    view = block[shift:].view(frames, V + pad)[:, :V]
    view.copy_(torch.from_numpy(img))
    return view


def _rows(ctx, rows, pad=0):
    """host rows [G][n] as a device tensor whose rows lie `pad` elements apart"""
    import torch
    t = _dev(ctx, rows)
    if not pad:
        return t
    big = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=t.dtype, device=ctx.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


# ------------------------------------------------------------------ (a) the f32 form
@pytest.mark.parametrize("G", [1, 5, 64, 1000, 4096])
@pytest.mark.parametrize("P", [1, 3, 10, 17, 64, 100, 300])
def test_f32_form_equals_the_numpy_loop(ctx, P, G):
    from zang_amd import zang
    if P * G > 1 << 20:
        pytest.skip("more than 2^20 voices")
    rng = np.random.default_rng(1000 * P + G)
    img = mg.image(rng, F, G * P, scale=5.0 / P ** 0.5, special_rate=0.004 / P)
    start = mg.image(rng, F, G, special_rate=0.004).T.copy()
    # a row pitch that allows 16-byte loads (where P does) for every other case, an odd one -- and a block that starts one float
    # past its alignment -- for the rest; dst rows padded too
    odd = (P + G) % 2 == 1
    src = _image(ctx, img, pad=5 if odd else 8, shift=1 if odd else 0)
    for span, zero_first in (((3, 1001), False), ((0, F), True), ((3, 1001), True), ((0, F), False)):
        dst = _rows(ctx, start, pad=3)
        zang.mixdownGroups(zang.Span(*span), dst, src, P, zero_first=zero_first, ctx=ctx)
        assert ctx.last_form() == ["k_mix_groups"]
        got = dst.cpu().numpy()
        assert mg.same_f32(got, mg.ref_sums(img, P, start, span, zero_first)), (span, zero_first)
    if G * P <= 1 << 16:                                            # and the plain image: rows back to back
        dst = _rows(ctx, start)
        zang.mixdownGroups(zang.Span(3, 1001), dst, _image(ctx, img), P, ctx=ctx)
        assert mg.same_f32(dst.cpu().numpy(), mg.ref_sums(img, P, start, (3, 1001), False))


# ------------------------------------------------------------------ (b) the PCM form
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("fmt", [S16, S8], ids=["s16", "s8"])
@pytest.mark.parametrize("P,G", [(1, 5), (3, 64), (10, 1000), (17, 5), (64, 64), (100, 5), (300, 5), (8, 4096)])
def test_pcm_form_equals_the_oracle_conversion_of_the_sums(ctx, oracle, P, G, fmt, nch):
    from zang_amd import zang
    rng = np.random.default_rng(77 * P + G + 10 * fmt + nch)
    img = mg.image(rng, F, G * P, scale=5.0 / P ** 0.5, special_rate=0.004 / P)
    acc = mg.image(rng, F, G, special_rate=0.004).T.copy()
    src = _image(ctx, img, pad=8 if G % 2 else 3)
    bps = 2 if fmt == S16 else 1
    prefill = rng.integers(0, 256, (G, F * nch * bps), dtype=np.uint8)
    for span, use_acc, ch, pad in (((3, 1001), True, nch - 1, 0), ((0, F), False, 0, 0), ((3, 1001), False, 0, 1), ((2, 1000), True, 0, 2)):
        sums = mg.ref_sums(img, P, acc, span, not use_acc)
        want = mg.ref_pcm(oracle, sums, span, fmt == S16, nch, ch, VOL, prefill)
        assert mg.pcm_arms(sums, span, fmt == S16, VOL) == mg.ALL_ARMS          # both clamps, NaN -> 0, truncation toward zero from both sides
        dst = _rows(ctx, prefill, pad=pad)                           # pad 1, 2: rows that do not start on a dword
        zang.mixdownGroupsPcm(zang.Span(*span), dst, src, P, fmt, nch, ch, VOL, acc=_rows(ctx, acc, pad=1) if use_acc else None, ctx=ctx)
        assert ctx.last_form() == ["k_mix_groups_pcm"]
        got = dst.cpu().numpy()
        assert np.array_equal(got, want), (span, use_acc, ch, pad, int((got != want).sum()))
        if nch == 2:                                                # the other channel's bytes are the prefill's
            other = np.ones(F * nch * bps, bool).reshape(F, nch, bps)
            other[:, ch, :] = False
            assert np.array_equal(got[:, other.reshape(-1)], prefill[:, other.reshape(-1)])


# ------------------------------------------------------------------ (c) the composition both forms replace
def _parent(ctx, src, P, span, start, zero_first, fmt, nch, ch, prefill):
    """zh_mixdown_voices(ZH_MIX_SEQUENTIAL) on every group's column view, then zh_mix_down: -> (f32 rows, PCM rows)"""
    import torch
    from zang_amd import zang
    G = src.shape[1] // P
    a, b = span
    bps = 2 if fmt == S16 else 1
    mix, pcm = _dev(ctx, start), _dev(ctx, prefill)
    for g in range(G):
        zang.mixdownVoices(zang.Span(a, b), mix[g], src[:, g * P:(g + 1) * P], zero_first=zero_first, sequential=True, ctx=ctx)
        zang.mixDown(pcm[g, a * nch * bps:b * nch * bps], mix[g, a:b], fmt, nch, ch, VOL, ctx=ctx)
    torch.cuda.synchronize()
    return mix.cpu().numpy(), pcm.cpu().numpy()


@pytest.mark.parametrize("P,G", [(3, 64), (17, 5), (100, 5), (10, 33), (300, 2), (1, 7)])
def test_both_forms_equal_the_per_group_composition(ctx, P, G):
    from zang_amd import zang
    rng = np.random.default_rng(5 * P + G)
    img = mg.image(rng, F, G * P, scale=5.0 / P ** 0.5, special_rate=0.004 / P)
    start = mg.image(rng, F, G, special_rate=0.004).T.copy()
    src = _image(ctx, img, pad=4)
    for span, zero_first, fmt, nch, ch in (((3, 1001), False, S16, 1, 0), ((0, F), True, S8, 2, 1), ((0, F), False, S16, 2, 0)):
        bps = 2 if fmt == S16 else 1
        prefill = rng.integers(0, 256, (G, F * nch * bps), dtype=np.uint8)
        want_f32, want_pcm = _parent(ctx, src, P, span, start, zero_first, fmt, nch, ch, prefill)
        dst = _rows(ctx, start)
        zang.mixdownGroups(zang.Span(*span), dst, src, P, zero_first=zero_first, ctx=ctx)
        assert mg.same_f32(dst.cpu().numpy(), want_f32)
        pcm = _rows(ctx, prefill)
        zang.mixdownGroupsPcm(zang.Span(*span), pcm, src, P, fmt, nch, ch, VOL, acc=None if zero_first else _rows(ctx, start), ctx=ctx)
        assert np.array_equal(pcm.cpu().numpy(), want_pcm)


# ------------------------------------------------------------------ (d) the acc chain over images of three kinds
@pytest.mark.parametrize("G", [1, 6, 200])
def test_acc_chain_over_three_images_equals_one_sequential_mix_of_17(ctx, oracle, G):
    import torch
    from zang_amd import zang
    rng = np.random.default_rng(17 + G)
    parts = [mg.image(rng, F, G * P, scale=1.2, special_rate=0.0005) for P in (3, 10, 4)]
    whole = np.concatenate([p.reshape(F, G, P) for p, P in zip(parts, (3, 10, 4))], axis=2).reshape(F, G * 17)
    span = (3, 1001)
    prefill = rng.integers(0, 256, (G, F * 2), dtype=np.uint8)
    zeros = np.zeros((G, F), np.float32)
    _, want = _parent(ctx, _image(ctx, whole), 17, span, zeros, True, S16, 1, 0, prefill)
    sums = mg.ref_sums(whole, 17, zeros, span, True)
    assert np.array_equal(want, mg.ref_pcm(oracle, sums, span, True, 1, 0, VOL, prefill))
    imgs = [_image(ctx, p, pad=pad) for p, pad in zip(parts, (1, 0, 4))]
    mix = torch.full((G, F), 99.0, dtype=torch.float32, device=ctx.device)
    pcm = _rows(ctx, prefill)
    sp = zang.Span(*span)
    zang.mixdownGroups(sp, mix, imgs[0], 3, zero_first=True, ctx=ctx)
    zang.mixdownGroups(sp, mix, imgs[1], 10, ctx=ctx)
    zang.mixdownGroupsPcm(sp, pcm, imgs[2], 4, S16, 1, 0, VOL, acc=mix, ctx=ctx)
    assert np.array_equal(pcm.cpu().numpy(), want)


# ------------------------------------------------------------------ (e) a captured graph: schedule + paint + grouped PCM mixdown
def test_captured_schedule_paint_and_grouped_pcm_replays_six_buffers(ctx):
    import torch
    import zang_amd
    from zang_amd import bank, modules as mod, zang
    P, n_inst, B = 8, 64, 6
    V = n_inst * P
    offsets, rec, t, ids = vb.corpus(n_inst, B)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                                    # (the legacy default stream cannot be captured)
    span = zang.Span(0, F)

    def kit(c):
        b = bank.VoiceBank(c, P, rec, offsets, t, ids, vb.ON_OFFSET, rows=34)
        return b, mod.NiceInstrument(V, 0.25, c), c.image(F, V), torch.zeros((n_inst, F * 2), dtype=torch.uint8, device=c.device), b.span_table(34, 0)
    be, me, ie, pe, te = kit(ctx)
    bg, mgr, ig, pg, tg = kit(c2)
    c2.sync()

    def body(b, m, img, pcm, table, c):
        b.schedule([F], vb.SR, 34)
        m.paint_spans(span, [img], None, vb.SR, table, zero_first=True)
        zang.mixdownGroupsPcm(span, pcm, img, P, S16, 1, 0, VOL, ctx=c)
    g = c2.capture(lambda: body(bg, mgr, ig, pg, tg, c2))          # recorded ONCE
    assert [k for k, _ in g.kernels()][-1] == "k_mix_groups_pcm"
    loud = False
    for bi in range(B):
        body(be, me, ie, pe, te, ctx)
        g.launch()
        ctx.sync(); c2.sync()
        a, b = pe.cpu().numpy(), pg.cpu().numpy()
        assert np.array_equal(a, b), bi
        loud = loud or bool(np.abs(a.view("<i2").astype(np.int32)).max() > 1000)
    assert loud and be.overflows() == 0 and bg.overflows() == 0
    g.close()
    be.close(); bg.close()
    c2.close()


# ------------------------------------------------------------------ (f) refusals
def test_refusals_return_their_codes_and_launch_nothing(ctx):
    import torch
    from zang_amd import abi, zang
    L, h = ctx.lib, ctx.handle
    G, P = 4, 3
    img = ctx.image(F, G * P, fill=1.0, pad=0)
    buf = zang.as_buf(img)
    dst = torch.full((G, F), 5.0, dtype=torch.float32, device=ctx.device)
    pcm = torch.full((G, F * 4), 0x5A, dtype=torch.uint8, device=ctx.device)
    zang.zero(zang.Span(0, 1), ctx.image(1, 1), ctx=ctx)
    marker = ctx.last_form()
    assert marker and "k_mix_groups" not in marker[0]
    bad, uns, ok = abi.ZH_ERR_INVALID, abi.ZH_ERR_UNSUPPORTED, abi.ZH_OK

    def f32(ctxh=h, s=0, e=F, d=dst.data_ptr(), stride=F, b=buf, p=P, flags=abi.PAINT_ZERO_FIRST):
        return L.zh_mixdown_groups(ctxh, s, e, d, stride, b, p, flags)

    def pc(ctxh=h, s=0, e=F, d=pcm.data_ptr(), stride=F * 4, b=buf, p=P, acc=dst.data_ptr(), acc_stride=F, fmt=S16, nch=2, ch=1):
        return L.zh_mixdown_groups_pcm(ctxh, s, e, d, stride, b, p, acc, acc_stride, fmt, nch, ch, VOL)

    def view(**kw):
        v = abi.Buf(buf.ptr, buf.voices, buf.frames, buf.stride, 0)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    for call in (f32, pc):
        assert call(ctxh=None) == bad and call(d=None) == bad and call(b=view(ptr=None)) == bad
        assert call(p=0) == bad and call(p=5) == bad and call(p=G * P + 1) == bad
        assert call(s=9, e=8) == bad and call(e=F + 1) == bad
        assert call(b=view(stride=G * P - 1)) == bad
        assert call(b=view(voices=0)) == ok and call(s=7, e=7) == ok            # no groups, an empty span: nothing to do
    assert f32(stride=F - 1) == bad and f32(s=3, e=100, stride=99) == bad and f32(s=3, e=100, stride=100) == ok
    assert f32(flags=abi.PAINT_TOLERANT) == uns and f32(flags=abi.PAINT_TOLERANT | abi.PAINT_ZERO_FIRST) == uns
    assert pc(stride=F * 4 - 1) == bad and pc(acc_stride=F - 1) == bad and pc(fmt=2) == bad and pc(nch=0) == bad and pc(ch=2) == bad
    assert pc(fmt=S8, stride=F * 2) == ok and pc(fmt=S8, stride=F * 2 - 1) == bad
    ctx.sync()
    # of everything above only four calls were valid and non-empty; undo them and look at what the refused ones left
    dst2 = torch.full((G, F), 5.0, dtype=torch.float32, device=ctx.device)
    pcm2 = torch.full((G, F * 4), 0x5A, dtype=torch.uint8, device=ctx.device)
    zang.zero(zang.Span(0, 1), ctx.image(1, 1), ctx=ctx)
    for call, d in ((lambda **kw: f32(d=dst2.data_ptr(), **kw), dst2), (lambda **kw: pc(d=pcm2.data_ptr(), **kw), pcm2)):
        before = d.clone()
        assert call(p=5) == bad and call(e=F + 1) == bad and call(s=7, e=7) == ok and call(b=view(voices=0)) == ok
        ctx.sync()
        assert torch.equal(d, before) and ctx.last_form() == marker
    assert f32(d=dst2.data_ptr(), flags=abi.PAINT_TOLERANT) == uns and pc(d=pcm2.data_ptr(), ch=2) == bad and pc(d=pcm2.data_ptr(), fmt=7) == bad
    ctx.sync()
    assert ctx.last_form() == marker and bool((dst2 == 5.0).all()) and bool((pcm2 == 0x5A).all())
    # one group: the stride is not looked at
    one = abi.Buf(buf.ptr, P, buf.frames, buf.stride, 0)
    assert L.zh_mixdown_groups(h, 0, F, dst2.data_ptr(), 0, one, P, abi.PAINT_ZERO_FIRST) == ok
    ctx.sync()
    assert ctx.last_form() == ["k_mix_groups"] and bool((dst2[0] == 3.0).all()) and bool((dst2[1:] == 5.0).all())
