"""Shared by the grouped-mixdown tests (host and GPU): seeded images with the awkward f32 values in them, the numpy statement of
the ordered f32 sum, and the oracle's mixDown applied row by row.  Not a test module."""
import ctypes as C

import numpy as np

f32 = np.float32
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-39, 1.4e-45, 3.0e38, -3.0e38, 1e30, -1e30], np.float32)


def image(rng, frames, voices, scale=1.0, special_rate=0.002):
    """[frames][voices] f32: uniform in (-scale, scale), a few cells replaced by NaN, +-inf, -0.0, denormals and huge values"""
    img = (rng.uniform(-1.0, 1.0, (frames, voices)) * scale).astype(np.float32)
    if special_rate:
        hit = rng.random((frames, voices)) < special_rate
        img[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
        for _ in range(3):                                          # and every one of them somewhere, whatever the rate
            img[rng.integers(0, frames, len(SPECIALS)), rng.integers(0, voices, len(SPECIALS))] = SPECIALS
    return img


def ref_sums(img, P, start_rows, span, zero_first):
    """rows [groups][frames]: inside the span s = start; s = s + voice k (k = 0 .. P-1), each add rounded to f32; outside it the
    start rows unchanged"""
    frames, V = img.shape
    G = V // P
    out = np.array(start_rows, np.float32, copy=True).reshape(G, frames)
    a, b = span
    s = np.zeros((G, b - a), np.float32) if zero_first else out[:, a:b].copy()
    with np.errstate(all="ignore"):
        for k in range(P):
            s = s + img[a:b, k::P].T                   # voice k of every group
            assert s.dtype == np.float32 and s.shape == (G, b - a)
    out[:, a:b] = s
    return out


def same_f32(a, b):
    """bit for bit, except that any NaN equals any NaN (the sign and payload of a NaN an add produces are the processor's choice)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def ref_pcm(oracle, sums, span, s16, num_channels, channel_index, vol, prefill):
    """the oracle's mixDown of every row's span into a copy of `prefill` [groups][frames * num_channels * bytes_per_sample]"""
    L = oracle.lib()
    fn = L.zo_mixdown_s16lsb if s16 else L.zo_mixdown_s8
    bps = 2 if s16 else 1
    out = np.array(prefill, np.uint8, copy=True)
    a, b = span
    for g in range(sums.shape[0]):
        row = np.ascontiguousarray(sums[g, a:b], np.float32)
        piece = np.ascontiguousarray(out[g, a * num_channels * bps:b * num_channels * bps])
        if b > a:
            fn(piece.ctypes.data_as(C.POINTER(C.c_uint8)), oracle.fptr(row), b - a, num_channels, channel_index, float(vol))
        out[g, a * num_channels * bps:b * num_channels * bps] = piece
    return out


def pcm_arms(sums, span, s16, vol):
    """which arms of mixDown the span's sums take: {"low", "high", "nan", "trunc_neg", "trunc_pos"} (for asserting coverage)"""
    a, b = span
    with np.errstate(all="ignore"):
        v = sums[:, a:b].astype(np.float32) * (f32(vol) * f32(32767.0 if s16 else 127.0))
    lo, hi = (-32767.0, 32766.0) if s16 else (-127.0, 126.0)
    arms = set()
    if (v <= lo).any():
        arms.add("low")
    if (v >= hi).any():
        arms.add("high")
    if np.isnan(v).any():
        arms.add("nan")
    mid = v[(v > lo) & (v < hi)]
    if ((mid < 0) & (mid != np.trunc(mid))).any():
        arms.add("trunc_neg")
    if ((mid > 0) & (mid != np.trunc(mid))).any():
        arms.add("trunc_pos")
    return arms


ALL_ARMS = {"low", "high", "nan", "trunc_neg", "trunc_pos"}
