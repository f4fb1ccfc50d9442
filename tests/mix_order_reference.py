"""The summation order of the voice mixdowns, restated in numpy float32: every add below is one IEEE f32 add (round to nearest even,
subnormals kept), in the order the kernels document.  No GPU, no library import: the constants are written out here with the
file:line they restate, so a kernel change that moves the order has to change this file on purpose.

  tree_mix   zh_mixdown_voices without ZH_MIX_SEQUENTIAL: k_mix_pass1 / k_mix_pass1_scalar + k_mix_pass2
             (zang_amd/csrc/basics.hip:168-282, the entry point :408-429)
  fused_mix  zh_nice_paint_mix / _stereo / _stereo_batch: the sum phase of k_nice_mix / k_nice_mix_batch + k_mix_pass2_wide
             (zang_amd/csrc/nice_mix.hip.h:111-160, zang_amd/csrc/basics.hip:284-315); its input is the per-voice image
             NiceInstrument.paint gives for the same script, which other tests hold to the oracle bit for bit

What no output can show, and the model therefore cannot pin: a partial sum's zero sign.  Both second passes start every chain at
+0.0f (basics.hip:268, :301), and +0.0 + (-0.0) = +0.0, x + (-0.0) = x + (+0.0) for every other x: whether a quad, a half row or
a tile partial came out -0.0 or +0.0 is gone before the destination is written.
"""
import numpy as np

F32 = np.float32

MIX_TILE = 1024          # basics.hip:174   voices per first-pass workgroup
MIX_LANES = 256          # basics.hip:183   __launch_bounds__(256): lane i owns voices 4 i .. 4 i + 3 of the tile (:187)
MIX_WAVE = 64            # basics.hip:177   wave_sum64
MIX_SHUFFLES = (32, 16, 8, 4, 2, 1)   # basics.hip:179   for (off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64)
MIX_SEG = 16             # basics.hip:260   second-pass segments

NICE_WAVE = 64           # nice_mix.hip.h:9    every wave (64 voices) works on its own
NICE_HALF = 32           # nice_mix.hip.h:12   lane (f, h) adds voices 32 h .. 32 h + 31 left to right (:119-128)
NICE_WG_WAVES = 4        # nice_mix.hip.h:152-154   ((w0 + w1) + w2) + w3; 256-thread workgroups (composite.hip:1446)
MIXW_SEG = 128           # basics.hip:291   1024 / 8 second-pass thread classes


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def _zeros(n):
    return np.zeros(n, F32)


# ------------------------------------------------------------------------------------------------ zh_mixdown_voices, tree form
def tree_tile_partials(src):
    """Pass 1 (basics.hip:183-217): src [V][F] -> partials [tiles][F]."""
    src = _f32(src)
    V, F = src.shape
    tiles = 0 if V == 0 else (V + MIX_TILE - 1) // MIX_TILE          # basics.hip:417
    partials = np.zeros((tiles, F), F32)
    for t in range(tiles):
        lane_sum = np.zeros((MIX_LANES, F), F32)                        # basics.hip:194   float s = 0.0f  (a dead quad stays +0.0)
        for i in range(MIX_LANES):
            v = t * MIX_TILE + 4 * i
            if v + 3 < V:                                               # basics.hip:196-198   a whole quad: no leading zero
                lane_sum[i] = ((src[v] + src[v + 1]) + src[v + 2]) + src[v + 3]
            elif v < V:                                                 # basics.hip:200   a quad cut by V: 0.0f, then += each live voice
                s = _zeros(F)
                for j in range(4):
                    if v + j < V:
                        s = s + src[v + j]
                lane_sum[i] = s
        x = lane_sum.reshape(MIX_LANES // MIX_WAVE, MIX_WAVE, F)        # [wave][lane][frame]
        lane = np.arange(MIX_WAVE)
        for off in MIX_SHUFFLES:                                        # basics.hip:179   all 64 lanes, every step
            x = x + x[:, lane ^ off, :]
        w = x[:, 0, :]                                                  # basics.hip:205-207   lane 0's value
        partials[t] = ((w[0] + w[1]) + w[2]) + w[3]                     # basics.hip:214
    return partials


def tree_mix(src, dst0, zero_first):
    """zh_mixdown_voices over a whole span: src [V][F] (the span's frames of every voice), dst0 [F] what the destination holds
    before.  Returns the destination after.  F = 0: the entry point returns before any launch (basics.hip:411).  V = 0: no
    first pass, the second pass runs over zero tiles (basics.hip:417-427): dst = (zero_first ? 0.0f : dst) + 0.0f."""
    src = _f32(src); dst0 = _f32(dst0)
    V, F = src.shape
    assert dst0.shape == (F,)
    if F == 0:
        return dst0.copy()
    partials = tree_tile_partials(src)
    tiles = partials.shape[0]
    per = (tiles + MIX_SEG - 1) // MIX_SEG                              # basics.hip:266
    seg = np.zeros((MIX_SEG, F), F32)
    for k in range(MIX_SEG):
        t0 = min(k * per, tiles); t1 = min(t0 + per, tiles)             # basics.hip:267
        s = _zeros(F)                                                   # basics.hip:268
        for t in range(t0, t1):                                         # basics.hip:272   tile order
            s = s + partials[t]
        seg[k] = s
    tot = seg[0]                                                        # basics.hip:277-279   all 16, the empty ones +0.0
    for k in range(1, MIX_SEG):
        tot = tot + seg[k]
    return ((_zeros(F) if zero_first else dst0) + tot).astype(F32)      # basics.hip:280   dst added last


def tree_mix_span(src, dst0, start, end, zero_first):
    """The entry point on a row: src [V][rows], dst0 [rows]; frames outside [start, end) keep their bits."""
    src = _f32(src); out = _f32(dst0).copy()
    out[start:end] = tree_mix(np.ascontiguousarray(src[:, start:end]), out[start:end], zero_first)
    return out


def sequential_mix(src, dst0, zero_first):
    """ZH_MIX_SEQUENTIAL (basics.hip:320-328), the order the tree form is told apart from: dst, then += voice 0, 1, 2, ..."""
    src = _f32(src); dst0 = _f32(dst0)
    s = _zeros(src.shape[1]) if zero_first else dst0.copy()
    for v in range(src.shape[0]):
        s = s + src[v]
    return s


# ------------------------------------------------------------------------------------------------ the fused NiceInstrument mixdown
def fused_rows(pv, gain, rows_per):
    """The sum phase of k_nice_mix for one channel: pv [F][V] per-voice samples, gain None (mono) or [V] / a scalar (the channel's
    per-voice gain) -> partial rows [rows][F]."""
    pv = _f32(pv)
    F, V = pv.shape
    blocks = (V + 255) // 256                                           # composite.hip:1446-1447
    Vp = blocks * 256
    x = np.zeros((F, Vp), F32)                                          # nice_mix.hip.h:166-174   lanes past V contribute +0.0
    x[:, :V] = pv
    if gain is not None:
        g = np.zeros(Vp, F32)                                           # nice_mix.hip.h:34   gains {0, 0} past the last voice
        g[:V] = np.broadcast_to(np.asarray(gain, F32), (V,))
        x = x * g[None, :]                                              # nice_mix.hip.h:123-128   the product rounded to f32, never fused
    h = x.reshape(F, Vp // NICE_HALF, NICE_HALF)
    s = h[:, :, 0].copy()                                               # nice_mix.hip.h:119, :126   the half's first voice, no leading zero
    for j in range(1, NICE_HALF):                                       # nice_mix.hip.h:121, :128   then += the next 31 in order
        s = s + h[:, :, j]
    wave = s[:, 0::2] + s[:, 1::2]                                      # nice_mix.hip.h:131-137   h0 + h1: [F][waves], dead waves included
    if rows_per == "wave":                                              # nice_mix.hip.h:133-139   blocks * 4 rows
        rows = wave
    else:
        assert rows_per == "workgroup", rows_per
        w = wave.reshape(F, blocks, NICE_WG_WAVES)
        rows = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]    # nice_mix.hip.h:152-154
    return np.ascontiguousarray(rows.T)


def wide_pass2(rows, dst0, zero_first):
    """k_mix_pass2_wide for one channel (basics.hip:294-315): rows [rows][F]."""
    R, F = rows.shape
    cls = np.zeros((MIXW_SEG, F), F32)                                  # basics.hip:301   every thread class starts at 0.0f
    for r0 in range(0, R, MIXW_SEG):                                    # basics.hip:305   class q adds rows q, q + 128, ...
        n = min(MIXW_SEG, R - r0)
        cls[:n] = cls[:n] + rows[r0:r0 + n]
    tot = cls[0]                                                        # basics.hip:310-312   s0 + s1 + ... + s127
    for k in range(1, MIXW_SEG):
        tot = tot + cls[k]
    return ((_zeros(F) if zero_first else dst0) + tot).astype(F32)      # basics.hip:313


def fused_mix(pv, gains, dst0, zero_first, rows_per):
    """zh_nice_paint_mix (gains None, dst0 [F]) or zh_nice_paint_mix_stereo (gains (left, right), each [V] or a scalar; dst0 a pair
    of [F]) over a whole span: pv [F][V].  Returns the destination(s) after; the two channels are independent.  V = 0: the entry
    point returns at once (composite.hip:1443); F = 0: no second pass (composite.hip:1494, :1498) -- nothing is written."""
    pv = _f32(pv)
    F, V = pv.shape
    if gains is None:
        dst0 = _f32(dst0)
        if V == 0 or F == 0:
            return dst0.copy()
        return wide_pass2(fused_rows(pv, None, rows_per), dst0, zero_first)
    out = []
    for g, d in zip(gains, dst0):
        d = _f32(d)
        out.append(d.copy() if V == 0 or F == 0 else wide_pass2(fused_rows(pv, g, rows_per), d, zero_first))
    return tuple(out)


def fused_mix_span(pv, gains, dst0, start, end, zero_first, rows_per):
    """The entry points on rows: pv [rows][V], dst0 [rows] (or a pair); frames outside [start, end) keep their bits."""
    pv = _f32(pv)
    if gains is None:
        out = _f32(dst0).copy()
        out[start:end] = fused_mix(pv[start:end], None, out[start:end], zero_first, rows_per)
        return out
    outs = tuple(_f32(d).copy() for d in dst0)
    got = fused_mix(pv[start:end], gains, tuple(o[start:end] for o in outs), zero_first, rows_per)
    for o, g in zip(outs, got):
        o[start:end] = g
    return outs


def rows_per_for(V, wg_min=65536):
    """Which row form the library takes (dispatch.hip:44 nice_mix_wg_min, composite.hip:1437)."""
    return "workgroup" if V >= int(wg_min) else "wave"
