"""GPU: the spectrum analyser (zh_fft, zh_spectrum_plot, zh_spectrum_column; csrc/spectrum.hip) against the yardstick
(tests/spectrum_reference.py), bit for bit, in every form the dispatch rows spectrum_tile / spectrum_stages select: the smallest
shapes at which the kernel can still go wrong -- every transform length class (one stage, an odd and an even number of stages, the
largest), voice counts around both tile widths and past one tile, a span that does not start at row 0 -- with canaries around
everything a call may write."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import spectrum_cases as sc
from tests import spectrum_reference as sr
from tests import util
from tests.hostile_cases import same_f32

pytestmark = pytest.mark.gpu
FORMS = [(16, 2), (8, 2), (16, 1), (8, 1)]
CANARY = 12345.5


def _form(monkeypatch, form):
    util.set_form(monkeypatch, spectrum_tile=form[0], spectrum_stages=form[1])


def _padded(ctx, frames, voices, pad=3):
    """(the whole tensor, canary-filled; its view of `voices` columns)"""
    import torch
    full = torch.full((frames, voices + pad), CANARY, dtype=torch.float32, device=ctx.device)
    return full, full[:, :voices]


@functools.lru_cache(maxsize=None)
def _pow10():
    from oracle import pyoracle
    return sr.oracle_pow10(pyoracle)


@functools.lru_cache(maxsize=None)
def _want_column(voices, height, logarithmic):
    return sr.column(sc.image(voices), height, logarithmic, _pow10())


@functools.lru_cache(maxsize=None)
def _want_plot(voices):
    return sr.plot(sc.image(voices))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [2, 4, 8, 64, 512, 1024])
def test_fft_in_place_equals_the_yardstick(ctx, monkeypatch, n, form):
    import torch
    from zang_amd import spectrum
    _form(monkeypatch, form)
    T = form[0]
    for V in (1, T - 1, T, T + 1, 130):
        for start in (0, 3):
            x = sc.image(V, seed=n + start, frames=2 * (n + 5))
            full_re, re = _padded(ctx, n + 5, V)
            full_im, im = _padded(ctx, n + 5, V)
            re.copy_(torch.from_numpy(x[:n + 5])); im.copy_(torch.from_numpy(x[n + 5:]))
            spectrum.fft(ctx, re, im, n, start)
            ctx.sync()
            assert ctx.last_form() == ["k_spectrum"]
            want_re, want_im = x[:n + 5].copy(), x[n + 5:].copy()
            r, i = np.ascontiguousarray(want_re[start:start + n]), np.ascontiguousarray(want_im[start:start + n])
            sr.fft(n, r, i)
            want_re[start:start + n], want_im[start:start + n] = r, i
            got_re, got_im = full_re.cpu().numpy(), full_im.cpu().numpy()
            assert same_f32(got_re[:, :V], want_re) and same_f32(got_im[:, :V], want_im), (n, V, start)     # rows outside the span too
            assert (got_re[:, V:] == CANARY).all() and (got_im[:, V:] == CANARY).all(), (n, V, start)


@pytest.mark.parametrize("form", FORMS)
def test_plot_equals_the_yardstick_on_the_case_table(ctx, monkeypatch, form):
    import torch
    from zang_amd import abi
    from zang_amd.runtime import as_buf
    _form(monkeypatch, form)
    V = 130
    img = torch.from_numpy(sc.image(V)).to(ctx.device)
    full, out = _padded(ctx, 520, V)
    runs = []
    for _ in range(2):
        abi.check(ctx.lib.zh_spectrum_plot(ctx.handle, 0, as_buf(img), as_buf(out)), "zh_spectrum_plot")
        ctx.sync()
        runs.append(full.cpu().numpy().copy())
    got = runs[0]
    assert same_f32(got[:512, :V], _want_plot(V))
    assert (got[512:] == CANARY).all() and (got[:, V:] == CANARY).all()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    assert abs(float(got[100, sc.case_voice("cosine")]) - 0.7071069) < 2e-7 and got[100, sc.case_voice("sine")] < 0.0045


@pytest.mark.parametrize("form", FORMS[:2])
def test_plot_on_views_with_an_odd_stride_and_a_misaligned_base(ctx, monkeypatch, form):
    import torch
    from zang_amd import spectrum
    _form(monkeypatch, form)
    V, stride, start = 130, 137, 3
    x = sc.image(V, frames=1024 + 5)
    flat = torch.full((1 + (1024 + 5) * stride,), CANARY, dtype=torch.float32, device=ctx.device)
    view = flat[1:].view(1024 + 5, stride)[:, :V]                       # the base one float past an aligned address, odd row stride
    assert view.data_ptr() % 8 == 4
    view.copy_(torch.from_numpy(x))
    before = flat.cpu().numpy().copy()
    s = spectrum.Spectrum(ctx, V)
    got = s.plot(view, start)
    ctx.sync()
    assert same_f32(got.cpu().numpy(), sr.plot(x[start:start + 1024]))
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), before.view(np.uint32))       # the samples are only read
    oflat = torch.full((1 + 512 * stride,), CANARY, dtype=torch.float32, device=ctx.device)
    oview = oflat[1:].view(512, stride)[:, :V]
    s.out = oview
    s.plot(view, start)
    ctx.sync()
    o = oflat.cpu().numpy()
    assert same_f32(o[1:].reshape(512, stride)[:, :V], sr.plot(x[start:start + 1024]))
    assert o[0] == CANARY and (o[1:].reshape(512, stride)[:, V:] == CANARY).all()


@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("logarithmic", [False, True])
@pytest.mark.parametrize("height", [2, 3, 128, 481])
def test_column_equals_the_yardstick(ctx, monkeypatch, height, logarithmic, form):
    import torch
    from zang_amd import abi
    from zang_amd.runtime import as_buf
    _form(monkeypatch, form)
    V, W = 130, 3
    img = torch.from_numpy(sc.image(V)).to(ctx.device)
    pixels = torch.full((height, W, V), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device)
    abi.check(ctx.lib.zh_spectrum_column(ctx.handle, 0, as_buf(img), C.c_void_p(pixels.data_ptr() + 4 * V), W * V, height, int(logarithmic)),
              "zh_spectrum_column")
    ctx.sync()
    got = pixels.cpu().numpy().view(np.uint32)
    want = _want_column(V, height, logarithmic)
    assert np.array_equal(got[:, 1, :], want), np.argwhere(got[:, 1, :] != want)[:5]
    assert (got[:, 0, :] == 0x5A5A5A5A).all() and (got[:, 2, :] == 0x5A5A5A5A).all()          # the neighbouring columns
    assert (got[:, 1, sc.case_voice("one_nan")] == 0xFFFF0000).all()


def test_full_grid_of_random_columns(ctx):
    import torch
    from zang_amd import spectrum
    V = 4096
    x = np.random.default_rng(4096).uniform(-1.0, 1.0, (1024, V)).astype(np.float32)
    got = spectrum.Spectrum(ctx, V).plot(torch.from_numpy(x).to(ctx.device))
    ctx.sync()
    idx = np.arange(63, V, 64)
    assert len(idx) == 64 and same_f32(got.cpu().numpy()[:, idx], sr.plot(np.ascontiguousarray(x[:, idx])))


def test_plot_recorded_into_a_graph_replays_on_changed_input(ctx):
    import torch
    import zang_amd
    from zang_amd import spectrum
    V = 33
    a, b = sc.image(V, seed=5), sc.image(V, seed=6)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                                       # binds to the side stream (capture needs a non-default stream)
        img = torch.from_numpy(a).to(c2.device)
        s = spectrum.Spectrum(c2, V)
        s.plot(img)                                                    # the context's table exists before the capture
        c2.sync()
        s.out.fill_(CANARY)
        g = c2.capture(lambda: s.plot(img))
        c2.sync()
        assert (s.out.cpu().numpy() == CANARY).all()                   # recording runs nothing
        replays = []
        for x in (a, b):
            img.copy_(torch.from_numpy(x))
            g.launch()
            c2.sync()
            replays.append(s.out.cpu().numpy().copy())
        eager = []
        for x in (a, b):
            img.copy_(torch.from_numpy(x))
            eager.append(s.plot(img).cpu().numpy().copy())
        g.close()
        c2.close()
    for r, e, x in zip(replays, eager, (a, b)):
        assert np.array_equal(r.view(np.uint32), e.view(np.uint32)) and same_f32(e, sr.plot(x))
    assert not np.array_equal(replays[0].view(np.uint32), replays[1].view(np.uint32))


def test_spectrogram_is_the_references_state_machine(ctx):
    """five buffers of a two-voice cosine sweep, width 4, the flip at the fourth buffer: the stored buffer and the picture in time
    order equal the reference class after every plot"""
    import torch
    from zang_amd import spectrum
    V, W, H = 2, 4, 37
    t = np.arange(5 * 1024)
    sweep = np.stack([np.cos(2 * np.pi * (20 + 0.01 * t) * t / 1024), 0.5 * np.cos(2 * np.pi * (200 - 0.015 * t) * t / 1024)], axis=1).astype(np.float32)
    img = torch.from_numpy(sweep).to(ctx.device)
    gram = spectrum.Spectrogram(ctx, V, W, H)
    ref = sr.Spectrogram(V, W, H, _pow10())
    for b in range(5):
        log = b >= 3
        gram.plot(img, frame_start=b * 1024, logarithmic=log)
        ref.plot(sweep[b * 1024:(b + 1) * 1024], log)
        ctx.sync()
        assert gram.drawindex == ref.drawindex and gram.logarithmic == ref.logarithmic
        assert np.array_equal(gram.buffer.cpu().numpy().view(np.uint32), ref.buffer), b
        assert np.array_equal(gram.scrolled().cpu().numpy().view(np.uint32), ref.scrolled()), b
    assert gram.drawindex == 2 and (ref.buffer[:, 2:] == 0).all() and (ref.buffer[:, :2] != 0).all()


def test_arguments_are_checked_on_the_device(ctx):
    import torch
    from zang_amd import abi
    from zang_amd.runtime import as_buf
    lib, h = ctx.lib, ctx.handle
    a, b, short, narrow = ctx.image(1024, 4, fill=0.0), ctx.image(1024, 4, fill=0.0), ctx.image(511, 4, fill=0.0), ctx.image(1024, 3, fill=0.0)
    px = torch.zeros((4, 4), dtype=torch.int32, device=ctx.device)
    p = C.c_void_p(px.data_ptr())
    inv = abi.ZH_ERR_INVALID
    for n in (0, 1, 3, 1000, 2048):
        assert lib.zh_fft(h, n, 0, as_buf(a), as_buf(b)) == inv
    assert lib.zh_fft(h, 1024, 1, as_buf(a), as_buf(b)) == inv and lib.zh_fft(h, 512, 513, as_buf(a), as_buf(b)) == inv     # rows outside
    assert lib.zh_fft(h, 2, 0xFFFFFFFF, as_buf(a), as_buf(b)) == inv
    assert lib.zh_fft(h, 512, 0, as_buf(a), as_buf(narrow)) == inv and lib.zh_fft(h, 512, 0, as_buf(a), as_buf(a)) == inv
    nul = abi.Buf(None, 4, 1024, 4, 0)
    assert lib.zh_fft(h, 512, 0, nul, as_buf(b)) == inv and lib.zh_spectrum_plot(h, 0, nul, as_buf(b)) == inv
    assert lib.zh_spectrum_plot(h, 1, as_buf(a), as_buf(b)) == inv and lib.zh_spectrum_plot(h, 0, as_buf(a), as_buf(short)) == inv
    assert lib.zh_spectrum_plot(h, 0, as_buf(a), as_buf(narrow)) == inv
    assert lib.zh_spectrum_column(h, 0, as_buf(a), None, 4, 4, 0) == inv and lib.zh_spectrum_column(h, 0, as_buf(a), p, 4, 1, 0) == inv
    assert lib.zh_spectrum_column(h, 0, as_buf(a), p, 3, 4, 0) == inv and lib.zh_spectrum_column(h, 1, as_buf(a), p, 4, 4, 0) == inv
    none = abi.Buf(None, 0, 0, 0, 0)
    assert lib.zh_fft(h, 1024, 0, none, none) == 0 and lib.zh_spectrum_plot(h, 0, none, none) == 0
    assert lib.zh_spectrum_column(h, 0, none, p, 0, 2, 1) == 0
    ctx.sync()
    assert (px.cpu().numpy() == 0).all() and (a.cpu().numpy() == 0).all()
    assert lib.zh_fft(h, 1024, 0, as_buf(a), as_buf(b)) == 0 and lib.zh_spectrum_column(h, 0, as_buf(a), p, 4, 4, 1) == 0
    ctx.sync()
