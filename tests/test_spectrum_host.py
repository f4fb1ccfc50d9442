"""CPU: the spectrum analyser without a device.  The surface -- the header, the ctypes mirror and the Zig binding declare the four
entry points, and every ZH_ERR_INVALID case that needs no device is refused -- the twiddle table against the yardstick on bits, the
per-element arithmetic of csrc/fft_lane.hip.h through a sanitized stand-alone harness against the yardstick on bits, the
yardstick's own checks, the case table, and Spectrogram's state rules over a fake library.

The harness (tests/cpp/fft_lane_host.cpp) covers the transform, the plot rows and the LINEAR column: the logarithmic position goes
through zmath.hip.h's pow, which is device code and does not compile for the host; the GPU tests hold the logarithmic column."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import spectrum_cases as sc
from tests import spectrum_reference as sr
from tests.hostile_cases import same_f32
from tests.hostprog import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zang_hip.h")
LANE_SRC = os.path.join(ROOT, "tests", "cpp", "fft_lane_host.cpp")

DECLS = [
    "ZH_API int zh_fft_twiddles(float *u, uint32_t n);",
    "ZH_API int zh_fft(zh_ctx *ctx, uint32_t n, uint32_t frame_start, zh_buf re, zh_buf im);",
    "ZH_API int zh_spectrum_plot(zh_ctx *ctx, uint32_t frame_start, zh_buf samples, zh_buf out);",
    "ZH_API int zh_spectrum_column(zh_ctx *ctx, uint32_t frame_start, zh_buf samples, uint32_t *pixels, size_t row_stride_pixels, "
    "uint32_t height, int logarithmic);",
]


# ------------------------------------------------------------------ surface
def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = " ".join(text.split()).replace(" ,", ",").replace(" )", ")")
    for decl in DECLS:
        assert " ".join(decl.split()) in text, decl


def test_ctypes_mirror_follows_the_header():
    import zang_amd
    from zang_amd import abi, spectrum
    P, vp, u32 = C.POINTER, C.c_void_p, C.c_uint32
    assert abi.SIGNATURES["zh_fft_twiddles"] == (C.c_int, [P(C.c_float), u32])
    assert abi.SIGNATURES["zh_fft"] == (C.c_int, [vp, u32, u32, abi.Buf, abi.Buf])
    assert abi.SIGNATURES["zh_spectrum_plot"] == (C.c_int, [vp, u32, abi.Buf, abi.Buf])
    assert abi.SIGNATURES["zh_spectrum_column"] == (C.c_int, [vp, u32, abi.Buf, vp, C.c_size_t, u32, C.c_int])
    assert abi.load().zh_spectrum_column.argtypes is not None
    assert zang_amd.Spectrum is spectrum.Spectrum and zang_amd.Spectrogram is spectrum.Spectrogram
    assert (spectrum.FRAMES, spectrum.BINS) == (sr.FRAMES, sr.BINS) == (1024, 512)


def test_zig_binding_declares_them():
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    assert "pub extern fn zh_fft_twiddles(u: ?[*]f32, n: u32) c_int;" in zig
    assert "pub extern fn zh_fft(ctx: ?*Ctx, n: u32, frame_start: u32, re: Buf, im: Buf) c_int;" in zig
    assert "pub extern fn zh_spectrum_plot(ctx: ?*Ctx, frame_start: u32, samples: Buf, out: Buf) c_int;" in zig
    assert ("pub extern fn zh_spectrum_column(ctx: ?*Ctx, frame_start: u32, samples: Buf, pixels: ?[*]u32, row_stride_pixels: usize, "
            "height: u32, logarithmic: c_int) c_int;") in zig


def test_bad_arguments_are_refused_without_a_device():
    """every ZH_ERR_INVALID case that is decided before a context is looked at: a NULL context and a NULL table, n that is no power
    of two or out of range"""
    from zang_amd import abi
    lib = abi.load()
    u = (C.c_float * 2048)()
    assert lib.zh_fft_twiddles(None, 1024) == abi.ZH_ERR_INVALID
    for n in (0, 1, 3, 6, 1000, 1023, 1025, 2048, 1 << 31):
        assert lib.zh_fft_twiddles(u, n) == abi.ZH_ERR_INVALID, n
    b = abi.Buf()
    px = (C.c_uint32 * 4)()
    assert lib.zh_fft(None, 1024, 0, b, b) == abi.ZH_ERR_INVALID
    assert lib.zh_spectrum_plot(None, 0, b, b) == abi.ZH_ERR_INVALID
    assert lib.zh_spectrum_column(None, 0, b, C.cast(px, C.c_void_p), 4, 2, 0) == abi.ZH_ERR_INVALID
    assert lib.zh_spectrum_column(None, 0, b, None, 4, 2, 0) == abi.ZH_ERR_INVALID


# ------------------------------------------------------------------ twiddles
def test_twiddle_table_is_the_references_on_bits_and_smaller_tables_are_prefixes():
    from zang_amd import abi
    lib = abi.load()
    want = sr.twiddles(1024)
    assert want.shape == (1023, 2) and want.nbytes == 8184
    full = np.zeros((1023, 2), np.float32)
    assert lib.zh_fft_twiddles(full.ctypes.data_as(C.POINTER(C.c_float)), 1024) == 0
    assert same_f32(full, want) and not np.isnan(full).any()
    assert (full[0] == (1.0, 0.0)).all() and (full[1] == (1.0, 0.0)).all() and full[2, 0] == np.float32(full[2, 0]) and full[2, 1] == -1.0
    for n in (2, 4, 8, 16, 32, 64, 128, 256, 512):
        part = np.full((n, 2), 7.0, np.float32)                        # one pair more than the call may write
        assert lib.zh_fft_twiddles(part.ctypes.data_as(C.POINTER(C.c_float)), n) == 0
        assert same_f32(part[:n - 1], full[:n - 1]) and (part[n - 1] == 7.0).all(), n
        assert same_f32(sr.twiddles(n), full[:n - 1])
    # the recurrence's own error: what no other FFT reproduces
    k = np.concatenate([np.arange(l) / (2.0 * l) for l in (1 << np.arange(10))])
    err = np.abs(full[:, 0] + 1j * full[:, 1] - np.exp(-2j * np.pi * k)).max()
    assert 1e-4 < err < 4e-4


# ------------------------------------------------------------------ the lane harness, sanitized
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(LANE_SRC, tmp_path_factory.mktemp("fft_lane"), ["-ffp-contract=off"])


def _run(exe, mode, head, arrays, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array(head, np.uint32).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip() == "PASS", r.stdout[-2000:] + r.stderr[-4000:]
    return np.fromfile(dst, np.uint32)


@pytest.mark.parametrize("n", [2, 4, 8, 64, 512, 1024])
def test_lane_harness_transform_equals_the_yardstick(harness, tmp_path, n):
    V = 17
    img = sc.image(V, seed=n, frames=2 * n)                            # the case columns' first frames, then random ones
    re, im = np.ascontiguousarray(img[:n]), np.ascontiguousarray(img[n:])
    got = _run(harness, "fft", [V, n], [re, im], tmp_path).view(np.float32).reshape(2, n, V)
    sr.fft(n, re, im)
    assert same_f32(got[0], re) and same_f32(got[1], im)
    assert np.isfinite(re[:, 0]).all() and np.abs(re[:, 0]).max() > 0


def test_lane_harness_plot_and_linear_column_equal_the_yardstick(harness, tmp_path):
    V, height = len(sc.NAMES) + 3, 481
    img = sc.image(V)
    words = _run(harness, "plot", [V, height], [img], tmp_path)
    rows = words[:512 * V].view(np.float32).reshape(512, V)
    pixels = words[512 * V:].reshape(height, V)
    assert same_f32(rows, sr.plot(img))
    assert np.array_equal(pixels, sr.column(img, height, False, None))
    for h in (2, 3):
        words = _run(harness, "plot", [V, h], [img], tmp_path)
        assert np.array_equal(words[512 * V:].reshape(h, V), sr.column(img, h, False, None)), h


# ------------------------------------------------------------------ the yardstick's own checks
def test_literal_bit_reversal_is_the_plain_permutation():
    for m in range(1, 11):
        n = 1 << m
        re = np.arange(n, dtype=np.float32).reshape(n, 1)
        im = -re
        sr.bit_reverse_literal(n, re, im)
        perm = sr.bit_reverse_permutation(n)
        assert np.array_equal(re[:, 0], perm) and np.array_equal(im[:, 0], -perm.astype(np.float32)), n
        assert np.array_equal(perm[perm], np.arange(n))               # an involution: storing row r AT perm[r] is the same move


def test_yardstick_stays_near_an_f64_fft():
    """within 1e-3 of the column's max|X| in either part: a few times what the twiddle recurrence costs (2.7e-4 measured on 130
    uniform columns at n = 1,024, seed 1).  The bound catches a wrong sign or stage order; it does not grade accuracy."""
    x = np.random.default_rng(1).uniform(-1.0, 1.0, (1024, 130)).astype(np.float32)
    for n in (2, 4, 8, 64, 512, 1024):
        re, im = np.ascontiguousarray(x[:n]), np.ascontiguousarray(x[1024 - n:][::-1])
        want = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64), axis=0)
        sr.fft(n, re, im)
        err = np.maximum(np.abs(re - want.real), np.abs(im - want.imag)).max(axis=0) / np.abs(want).max(axis=0)
        print(n, err.max())
        assert err.max() < 1e-3, (n, err.max())


def test_real_part_only_quirk_is_pinned():
    """both widgets read fft_real alone: a cosine on bin 100 peaks at 0.7071069 there, a sine on bin 100 shows next to nothing at
    its own bin while |fft_imag[100]| is 512"""
    cos, sin = sc.column("cosine")[:, None], sc.column("sine")[:, None]
    p = sr.plot(cos)[:, 0]
    assert p.argmax() == 100 and abs(float(p[100]) - 0.7071069) < 2e-7 and round(float(np.delete(p, 100).max()), 4) <= 0.0012
    q = sr.plot(sin)[:, 0]
    assert q[100] <= 0.0045
    re, im = np.ascontiguousarray(sin), np.zeros_like(sin)
    sr.fft(1024, re, im)
    assert abs(abs(float(im[100, 0])) - 512.0) < 0.5 and abs(float(re[100, 0])) < 0.03


def test_defined_casts_and_colours():
    big = np.array([np.nan, -1.0, -0.0, 0.0, 0.99, 1.0, 255.9, 4294967040.0, 4294967296.0, np.inf, -np.inf], np.float32)
    assert sr.to_u32(big).tolist() == [0, 0, 0, 0, 0, 1, 255, 4294967040, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    assert sr.pixel(np.array([np.nan], np.float32))[0] == 0xFFFF0000
    assert sr.pixel(np.array([0.0, -0.0], np.float32)).tolist() == [0xFF000000, 0xFF000000]
    assert sr.pixel(np.array([np.inf], np.float32))[0] == 0xFF000000          # sqrt(inf) times a zero channel is NaN, which casts to 0
    loud = sr.pixel(np.array([1536.0], np.float32))[0]                        # h = 1.2247: green is 282, its ninth bit lands in blue
    assert (int(loud) >> 16) & 0xFF == ((int(sr.to_u32(np.float32(0))) | 1)) and int(loud) >> 24 == 0xFF
    with pytest.raises(ValueError):
        sr.column(np.zeros((1024, 1), np.float32), 1, False, None)
    for n in (0, 1, 3, 12):
        with pytest.raises(ValueError):
            sr.twiddles(n)


# ------------------------------------------------------------------ the case table
def test_the_test_tables_reach_every_case_the_issue_names(oracle):
    assert sc.NAMES == ["random", "zero", "dc", "nyquist", "impulse_first", "impulse_last", "cosine", "sine", "negative_zero", "denormal",
                        "one_inf", "one_nan", "huge", "overflow", "loud"]
    img = sc.image(130)
    col = lambda name: img[:, sc.case_voice(name)]
    assert img.shape == (1024, 130) and img.dtype == np.float32 and len(sc.NAMES) < 16 < 130       # the cases sit in the first tile
    assert np.abs(col("random")).max() <= 1.0 and len(set(col("random").tolist())) > 1000
    assert (col("zero").view(np.uint32) == 0).all() and (col("negative_zero").view(np.uint32) == 0x80000000).all()
    assert (col("dc") == 1.0).all() and (col("nyquist")[0::2] == 1.0).all() and (col("nyquist")[1::2] == -1.0).all()
    assert col("impulse_first")[0] == 1.0 and np.count_nonzero(col("impulse_first")) == 1
    assert col("impulse_last")[1023] == 1.0 and np.count_nonzero(col("impulse_last")) == 1
    den = col("denormal")
    assert np.count_nonzero(den) == 1 and 0 < den.max() < np.finfo(np.float32).tiny
    assert np.isinf(col("one_inf")).sum() == 1 and np.isnan(col("one_nan")).sum() == 1
    assert (col("huge") == np.float32(1e30)).all() and (col("overflow") == np.float32(1e36)).all()
    re = sr.fft_real(img)
    assert re[0, sc.case_voice("huge")] == np.float32(1.024e33)                # 1e30 alone stays finite: the next case overflows
    assert not np.isfinite(re[0, sc.case_voice("overflow")]) and np.isnan(re[:, sc.case_voice("one_nan")]).all()
    assert np.isnan(re[:, sc.case_voice("one_inf")]).any()
    assert np.abs(re[:512, sc.case_voice("loud")]).max() > 1024                # hslToRgb sees h > 1 ...
    for log in (False, True):
        px = sr.column(img, 128, log, sr.oracle_pow10(oracle))
        loud = px[:, sc.case_voice("loud")].astype(np.int64)
        assert (px >> 24 == 0xFF).all()
        assert (px[:, sc.case_voice("one_nan")] == 0xFFFF0000).all()
        # ... and a channel above 255 spills into the next byte: green's ninth bit sets blue's lowest where blue itself is zero
        h = sr.plot_value(np.float32(1536.0))
        assert h > 1 and any((w >> 16) & 0xFF == 1 and (w >> 8) & 0xFF > 0 for w in loud.tolist())
        assert len(set(px[:, sc.case_voice("random")].tolist())) > 64
    assert (sr.column(img, 128, False, None) != sr.column(img, 128, True, sr.oracle_pow10(oracle))).any()


# ------------------------------------------------------------------ Spectrogram's state rules, no device
class _FakeLib:
    """stands in for libzang_hip.so: zh_spectrum_column writes the call's ordinal down the column it was pointed at"""

    def __init__(self, owner):
        self.owner, self.calls = owner, []

    def zh_spectrum_column(self, handle, frame_start, buf, pixels, row_stride, height, logarithmic):
        g = self.owner
        at = (pixels.value - g.buffer.data_ptr()) // 4
        assert at % g.voices == 0 and row_stride == g.width * g.voices and height == g.height
        self.calls.append((frame_start, at // g.voices, logarithmic))
        g.buffer[:, at // g.voices, :] = len(self.calls)
        return 0


def _fake_spectrogram(voices, width, height):
    import torch
    from zang_amd import spectrum

    class _Ctx:
        handle = None
    g = object.__new__(spectrum.Spectrogram)
    g.ctx, g.voices, g.width, g.height = _Ctx(), voices, width, height
    g.logarithmic, g.drawindex = False, 0
    g.buffer = torch.zeros((height, width, voices), dtype=torch.int32)
    g.ctx.lib = _FakeLib(g)
    return g


def test_spectrogram_state_rules_without_a_device():
    from zang_amd import abi
    g = _fake_spectrogram(2, 4, 3)
    img = abi.Buf()
    cols = lambda: g.buffer[0, :, 0].tolist()
    for k in range(1, 4):
        g.plot(img, frame_start=k)
    assert cols() == [1, 2, 3, 0] and g.drawindex == 3
    assert g.scrolled()[0, :, 0].tolist() == [0, 1, 2, 3]                       # the oldest column first, the newest last
    g.plot(img)
    assert cols() == [1, 2, 3, 4] and g.drawindex == 0                          # wraps at width
    g.plot(img)
    assert cols() == [5, 2, 3, 4] and g.drawindex == 1 and g.scrolled()[1, :, 1].tolist() == [2, 3, 4, 5]
    g.plot(img, logarithmic=True)                                               # a flip clears and resets BEFORE the column is drawn
    assert cols() == [6, 0, 0, 0] and g.drawindex == 1 and g.logarithmic is True
    g.plot(img, logarithmic=True)
    assert cols() == [6, 7, 0, 0] and g.drawindex == 2
    g.plot(img, logarithmic=False)
    assert cols() == [8, 0, 0, 0] and g.scrolled()[2, :, 0].tolist() == [0, 0, 0, 8]
    assert [c[1] for c in g.ctx.lib.calls] == [0, 1, 2, 3, 0, 0, 1, 0] and [c[2] for c in g.ctx.lib.calls] == [0, 0, 0, 0, 0, 1, 1, 0]
    assert [c[0] for c in g.ctx.lib.calls[:3]] == [1, 2, 3]
    # the yardstick's class follows the same rules
    ref = sr.Spectrogram(1, 4, 2, None)
    x = sc.image(1)
    for log in (False,) * 5:
        ref.plot(x, log)
    assert ref.drawindex == 1 and (ref.buffer != 0).all()
    assert np.array_equal(ref.scrolled()[:, 3], ref.buffer[:, 0])
