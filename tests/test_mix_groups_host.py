"""CPU: the grouped voice mixdown's surface and its per-sample arithmetic.  include/zang_hip.h declares zh_mixdown_groups /
zh_mixdown_groups_pcm, the ctypes mirror and the Zig binding list them; zang_amd/csrc/mix_lane.hip.h -- the text the kernels run
per (group, frame) -- is compiled for the host with AddressSanitizer + UBSan (tests/cpp/mix_lane_host.cpp) and held against a
numpy f32 add-by-add loop and the oracle's mixDown.  No tolerance: ordered f32 adds, one multiply, an integer conversion."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mix_groups_cases as mg
from tests.hostprog import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mix_lane_host.cpp")

DECLS = {
    "zh_mixdown_groups": "ZH_API int zh_mixdown_groups(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, float *dst, size_t dst_stride_floats, "
                         "zh_buf src, uint32_t group_voices, uint32_t flags);",
    "zh_mixdown_groups_pcm": "ZH_API int zh_mixdown_groups_pcm(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, uint8_t *dst, size_t dst_stride_bytes, "
                             "zh_buf src, uint32_t group_voices, const float *acc, size_t acc_stride_floats, "
                             "uint32_t audio_format, uint32_t num_channels, uint32_t channel_index, float vol);",
}


def test_header_mirror_and_binding_declare_the_two_entry_points():
    from zang_amd import abi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "zang_hip.h")).read(), flags=re.S)
    text = " ".join(text.split()).replace(" ,", ",")           # (a comment after a parameter leaves a blank before its comma)
    for name, decl in DECLS.items():
        assert " ".join(decl.split()) in text, name
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    assert abi.SIGNATURES["zh_mixdown_groups"] == (C.c_int, [vp, u32, u32, vp, sz, abi.Buf, u32, u32])
    assert abi.SIGNATURES["zh_mixdown_groups_pcm"] == (C.c_int, [vp, u32, u32, vp, sz, abi.Buf, u32, vp, sz, u32, u32, u32, C.c_float])
    lib = abi.load()
    assert lib.zh_mixdown_groups.argtypes is not None and lib.zh_mixdown_groups_pcm.argtypes is not None
    zig = open(os.path.join(ROOT, "bindings", "zang_hip.zig")).read()
    assert "pub extern fn zh_mixdown_groups(ctx: ?*Ctx, span_start: u32, span_end: u32, dst: ?[*]f32, dst_stride_floats: usize, src: Buf, " \
           "group_voices: u32, flags: u32) c_int;" in zig
    assert "pub extern fn zh_mixdown_groups_pcm(ctx: ?*Ctx, span_start: u32, span_end: u32, dst: ?[*]u8, dst_stride_bytes: usize, src: Buf, " \
           "group_voices: u32, acc: ?[*]const f32, acc_stride_floats: usize, audio_format: u32, num_channels: u32, channel_index: u32, vol: f32) c_int;" in zig


def test_refusals_that_need_no_device():
    """a NULL context is refused before anything else is looked at"""
    from zang_amd import abi
    lib = abi.load()
    assert lib.zh_mixdown_groups(None, 0, 0, None, 0, abi.Buf(), 1, 0) == abi.ZH_ERR_INVALID
    assert lib.zh_mixdown_groups_pcm(None, 0, 0, None, 0, abi.Buf(), 1, None, 0, 1, 1, 0, 0.25) == abi.ZH_ERR_INVALID


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("mix_lane"))


def _through_harness(exe, tmp, img, stride, P, start_rows, span, zero_first, s16, nch, ch, vol):
    frames, V = img.shape
    G = V // P
    padded = np.full((frames, stride), np.float32(777.0), np.float32)          # what lies between the rows is never added
    padded[:, :V] = img
    flat = padded.reshape(-1)[:(frames - 1) * stride + V]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([G, P, frames, stride, span[0], span[1], int(zero_first), int(s16), nch, ch, np.float32(vol).view(np.uint32)], np.uint32).tobytes())
        f.write(flat.tobytes() + np.ascontiguousarray(start_rows, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(fout, "rb").read()
    bps = 2 if s16 else 1
    sums = np.frombuffer(raw, np.float32, G * frames).reshape(G, frames)
    pcm = np.frombuffer(raw, np.uint8, G * frames * nch * bps, G * frames * 4).reshape(G, frames * nch * bps)
    assert G * frames * 4 + pcm.size == len(raw)
    return sums, pcm


CASES = [  # groups, P, frames, row stride, span, zero_first, s16, channels, channel, scale of the samples
    (1, 1, 64, 1, (0, 64), True, True, 1, 0, 2.0),
    (5, 3, 200, 15, (3, 197), True, True, 1, 0, 3.0),
    (7, 10, 129, 96, (0, 129), False, True, 2, 1, 1.0),
    (4, 17, 100, 68, (1, 99), False, False, 1, 0, 1.5),
    (3, 64, 70, 200, (0, 70), True, False, 2, 0, 0.2),
    (2, 300, 40, 601, (5, 40), False, True, 3, 2, 0.05),
    (6, 4, 50, 24, (10, 10), True, True, 1, 0, 1.0),                           # an empty span: nothing changes
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "g%d_p%d_%s%dch" % (c[0], c[1], "s16_" if c[6] else "s8_", c[7]))
def test_lane_arithmetic_equals_numpy_adds_and_the_oracle_conversion(harness, oracle, tmp_path, case):
    G, P, frames, stride, span, zero_first, s16, nch, ch, scale = case
    rng = np.random.default_rng(20260117 + G * 1000 + P)
    vol = 0.25
    # samples sized so that vol * 32767 (or 127) * sum straddles both clamps; specials at a rate that leaves most sums finite
    img = mg.image(rng, frames, G * P, scale=scale * 4.0 / max(P, 1) ** 0.5, special_rate=0.01 / max(P, 1) ** 0.5)
    start_rows = mg.image(rng, frames, G, scale=1.0, special_rate=0.01).T.copy()
    sums, pcm = _through_harness(harness, str(tmp_path), img, stride, P, start_rows, span, zero_first, s16, nch, ch, vol)
    ref = mg.ref_sums(img, P, start_rows, span, zero_first)
    assert mg.same_f32(sums, ref)
    bps = 2 if s16 else 1
    ref_pcm = mg.ref_pcm(oracle, ref, span, s16, nch, ch, vol, np.full((G, frames * nch * bps), 0xAA, np.uint8))
    assert np.array_equal(pcm, ref_pcm)
    if span[1] - span[0] >= 64 and P <= 64:
        assert {"low", "high", "trunc_neg", "trunc_pos"} <= mg.pcm_arms(ref, span, s16, vol), mg.pcm_arms(ref, span, s16, vol)


def test_conversion_edges_equal_the_oracle(harness, oracle, tmp_path):
    """one group of one voice, zero-first: the sum IS the sample, so every edge of the conversion is hit by construction"""
    vol = 0.25
    for s16 in (True, False):
        mul = np.float32(vol) * np.float32(32767.0 if s16 else 127.0)
        lo, hi = (-32767.0, 32766.0) if s16 else (-127.0, 126.0)
        edges = []
        for t in (lo, hi, lo + 1, hi - 1, 0.0, -0.0, 0.999, -0.999, 1.0, -1.0, 1.5, -1.5, 2.5, -2.5, lo - 0.5, lo + 0.5, hi - 0.5, hi + 0.5, 100.7, -100.7):
            x = np.float32(t) / mul
            edges += [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
        samples = np.concatenate([np.array(edges, np.float32), mg.SPECIALS])
        img = samples.reshape(-1, 1)
        n = len(samples)
        sums, pcm = _through_harness(harness, str(tmp_path), img, 1, 1, np.zeros((1, n), np.float32), (0, n), True, s16, 1, 0, vol)
        assert mg.same_f32(sums[0], np.float32(0.0) + samples)
        ref = mg.ref_pcm(oracle, sums, (0, n), s16, 1, 0, vol, np.zeros((1, n * (2 if s16 else 1)), np.uint8))
        assert np.array_equal(pcm, ref)
        assert mg.pcm_arms(sums, (0, n), s16, vol) == mg.ALL_ARMS
