"""GPU parity: the device's std.math.pow with its logf and expf (csrc/zmath.hip.h zpowf_pos / zpowf / zlogf / zexpf) against the
oracle's restatement (zo_math_powf_n), bit for bit, through both builds of the header: zh_pow (hipcc, k_pow -> zpowf_pos) and a
generated script kernel (hiprtc, the embedded copy -> zpowf).  No tolerance anywhere: the NaN masks are equal and every other
value is equal as uint32, so the sign of a zero counts.

The inputs come from tests/pow_cases.py, which also sorts every pair -- from the inputs and the oracle's result alone -- into the
leaves of the four routines and asserts a count for each (tests/test_pow_corpus.py runs the same condition without a GPU).
Leaves no argument of pow reaches (pow_cases.UNREACHABLE): zexpf's ldexpf into the subnormals and its range tests between
0x42aeac50 and the overflow / underflow thresholds (the fractional path's product is below 52 in magnitude, the yi >= 2^31 path's
at least 128); zexpf's NaN argument and zlogf's returns for 0, inf and 1 (zpowf's tables answer those first).  Subnormal results of
pow itself come from the ldexpf at the end of zpowf / zpowf_pos, and are reached by half a million pairs.

A script's paint ADDS into its output, and 0 + (-0) == +0: an image of zeros would hide the sign of a zero result.  The images
here start at -0.0, for which -0 + r == r for every r, both zeros included."""
import time

import numpy as np
import pytest

from tests import pow_cases as pc

pytestmark = pytest.mark.gpu
SR = 48000.0
SCRIPT = """
PowBB = defmodule x: waveform, y: waveform, begin out pow(x, y) end
PowBC = defmodule x: waveform, y: constant, begin out pow(x, y) end
PowCB = defmodule x: constant, y: waveform, begin out pow(x, y) end
PowCC = defmodule x: constant, y: constant, begin out pow(x, y) end
"""


def _differing(x, y, got, ref):
    """-> (pairs that differ, a few of them): NaN where the oracle has NaN and nowhere else, every other value the same bits"""
    nan = np.isnan(ref)
    bad = np.nonzero((np.isnan(got) != nan) | ((got.view(np.uint32) != ref.view(np.uint32)) & ~nan))[0]
    return bad.size, [(hex(int(pc.bits(x[i:i + 1])[0])), hex(int(pc.bits(y[i:i + 1])[0])), hex(int(got[i:i + 1].view(np.uint32)[0])),
                       hex(int(ref[i:i + 1].view(np.uint32)[0]))) for i in bad[:6]]


# ------------------------------------------------------------------ zh_pow: finite x > 0, any y
def test_zh_pow_bitexact(ctx, oracle):
    """every group of pow_cases.positive_groups through zh_pow; the corpus reaches every leaf of pow_cases.POSITIVE_LEAVES"""
    import torch
    from zang_amd import abi
    pc.assert_reached(pc.positive_counts(oracle)[0], pc.POSITIVE_LEAVES)
    failures, pairs, t0 = [], 0, time.time()
    for name, x, y in pc.positive_groups(oracle):
        ref = pc.oracle_pow(oracle, x, y)
        xd, yd = torch.from_numpy(x.copy()).to(ctx.device), torch.from_numpy(y.copy()).to(ctx.device)
        out = torch.empty_like(xd)
        abi.check(ctx.lib.zh_pow(ctx.handle, x.size, out.data_ptr(), xd.data_ptr(), yd.data_ptr()), "zh_pow")
        ctx.sync()
        n, some = _differing(x, y, out.cpu().numpy(), ref)
        print("zh_pow / %s: %d pairs, %d differ" % (name, x.size, n))
        pairs += x.size
        if n:
            failures.append((name, n, some))
    print("zh_pow: %d pairs in %.1f s" % (pairs, time.time() - t0))
    assert not failures, failures
    assert pairs >= (1 << 24) + (8 << 20)


def test_zh_pow_rejects_null(ctx):
    assert ctx.lib.zh_pow(ctx.handle, 0, None, None, None) == 0
    assert ctx.lib.zh_pow(ctx.handle, 4, None, None, None) != 0


# ------------------------------------------------------------------ zpowf through a generated kernel: all of IEEE
@pytest.fixture(scope="module")
def program(ctx):
    from zang_amd import script
    p = script.ScriptProgram(SCRIPT, ctx, filename="pow.txt")
    yield p
    p.close()


def test_generated_kernels_call_zpowf(program):
    """each of the four arithmetic kinds of the emitter (buffer-buffer, buffer-float, float-buffer, float-float) calls zpowf"""
    import re
    kernels = [(re.search(r"\b(zs_\w+)\(const ZsLaunch", k), k) for k in program.hip_source.split('extern "C" __global__')]
    for name in ("PowBB", "PowBC", "PowCB", "PowCC"):
        paints = [k for h, k in kernels if h and h.group(1).startswith("zs_paint") and h.group(1).endswith("_" + name)]
        assert paints and all("zpowf(" in k for k in paints), name
    assert "zpowf(x[0], x[1])" in program.hip_source and "zpowf(P1, P2)" in program.hip_source


def _paint(ctx, m, F, V, params):
    from zang_amd import zang
    out = ctx.image(F, V, fill=-0.0)                              # -0 + r == r: the sign of a zero result survives the add
    m.paint(zang.Span(0, F), [out], [], False, dict(params, sample_rate=SR))
    ctx.sync()
    return out.cpu().numpy().reshape(-1)


@pytest.mark.parametrize("V", [70, 4096])
def test_script_pow_buffers_bitexact(ctx, oracle, program, V):
    """PowBB over pow_cases.any_groups: V = 70 is one full wave and a partial one, V = 4,096 sixty-four waves; a paint holds
    ceil(2^20 / V) frames, so a full one evaluates at least 2^20 pairs.  The corpus reaches every leaf of pow_cases.ANY_LEAVES."""
    import torch
    pc.assert_reached(pc.any_counts(oracle)[0], pc.ANY_LEAVES)
    assert np.signbit(ctx.image(2, V, fill=-0.0).cpu().numpy()).all()
    F = -(-(1 << 20) // V)
    m = program.module("PowBB", V)
    failures, pairs, full, t0 = [], 0, 0, time.time()
    for name, x, y in pc.any_groups(oracle):
        ref = pc.oracle_pow(oracle, x, y)
        differ, some = 0, []
        for a in range(0, x.size, F * V):
            b = min(a + F * V, x.size)
            Fb = -(-(b - a) // V)
            xp, yp = np.ones(Fb * V, np.float32), np.ones(Fb * V, np.float32)           # (the last rows' spare voices: pow(1, 1))
            xp[:b - a] = x[a:b]; yp[:b - a] = y[a:b]
            got = _paint(ctx, m, Fb, V, {"x": torch.from_numpy(xp.reshape(Fb, V)).to(ctx.device), "y": torch.from_numpy(yp.reshape(Fb, V)).to(ctx.device)})
            n, s = _differing(x[a:b], y[a:b], got[:b - a], ref[a:b])
            differ += n; some += s
            full += Fb == F
        print("PowBB V=%d / %s: %d pairs, %d differ" % (V, name, x.size, differ))
        pairs += x.size
        if differ:
            failures.append((name, differ, some[:6]))
    m.close()
    print("PowBB V=%d: %d pairs in %.1f s" % (V, pairs, time.time() - t0))
    assert not failures, failures
    assert full >= 16 and F * V >= 1 << 20 and pairs >= 2 * ((1 << 24) + (8 << 20)) + (2 << 20)


def _constant_side():
    """4,096 random pairs for the constant forms: half random bit patterns, half the wide recipe with x of both signs and y one
    third integers"""
    rng = np.random.default_rng(20261018)
    n = 2048
    x = np.concatenate([pc.fl(rng.integers(0, 1 << 32, n, dtype=np.uint64)), pc.wide_x(rng, n) * rng.choice(np.array([-1, 1], np.float32), n)])
    yw = pc.wide_y(rng, n)
    yw[::3] = rng.integers(-300, 301, yw[::3].size).astype(np.float32)
    y = np.concatenate([pc.fl(rng.integers(0, 1 << 32, n, dtype=np.uint64)), yw])
    p = rng.permutation(2 * n)
    return x[p].astype(np.float32), y[p].astype(np.float32)


@pytest.mark.parametrize("V", [70, 4096])
def test_script_pow_constant_forms_bitexact(ctx, oracle, program, V):
    """PowBC, PowCB, PowCC: one value per voice on the constant side (V distinct constants a paint), crossed with the frames of
    the waveform side -- the full cross product of pow_cases.X_CROSS and Y_CROSS and 4,096 random pairs; a hoisted or differently
    emitted constant path (csrc/zscript_emit.hip treats pow on its own) would show here"""
    import torch
    xs, ys = pc.fl(pc.X_CROSS), pc.fl(pc.Y_CROSS)
    rx, ry = _constant_side()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(ctx.device)
    failures = []

    def run(name, consts, frames, build):
        """`consts`: the values of the constant side, V a paint (the last paint wraps round); `frames`: the waveform side's values,
        every voice sees all of them, each voice starting at another; build(c [V], w [F][V] or None) -> (params, x, y) flat"""
        m = program.module(name, V)
        pairs = differ = 0
        some = []
        for a in range(0, len(consts[0]), V):
            c = [np.take(k, np.arange(a, a + V), mode="wrap") for k in consts]
            Fn = len(frames) if frames is not None else 8
            w = frames[(np.arange(Fn)[:, None] + np.arange(V)[None, :]) % Fn] if frames is not None else None
            params, x, y = build(c, w, Fn)
            got = _paint(ctx, m, Fn, V, params)
            n, s = _differing(x, y, got, pc.oracle_pow(oracle, x, y))
            pairs += x.size; differ += n; some += s
        m.close()
        print("%s V=%d: %d pairs, %d differ" % (name, V, pairs, differ))
        if differ:
            failures.append((name, differ, some[:6]))
        return pairs

    flat = lambda a, Fn: np.ascontiguousarray(np.broadcast_to(a, (Fn, V))).reshape(-1)
    # PowBC: x the waveform (X_CROSS and 47 random values: 64 frames), y per voice (Y_CROSS, then the random ones)
    n_bc = run("PowBC", [np.concatenate([ys, ry])], np.concatenate([xs, rx[:64 - xs.size]]),
               lambda c, w, Fn: ({"x": dev(w), "y": dev(c[0])}, w.reshape(-1), flat(c[0], Fn)))
    # PowCB: x per voice (X_CROSS, then the random ones), y the waveform (Y_CROSS and 37 random values: 64 frames)
    n_cb = run("PowCB", [np.concatenate([xs, rx])], np.concatenate([ys, ry[:64 - ys.size]]),
               lambda c, w, Fn: ({"x": dev(c[0]), "y": dev(w)}, flat(c[0], Fn), w.reshape(-1)))
    # PowCC: both per voice -- the cross product pair by pair, then the random pairs; every frame of the voice holds pow(x, y)
    cx, cy = pc.cross_product()
    n_cc = run("PowCC", [np.concatenate([cx, rx]), np.concatenate([cy, ry])], None,
               lambda c, w, Fn: ({"x": dev(c[0]), "y": dev(c[1])}, flat(c[0], Fn), flat(c[1], Fn)))
    assert not failures, failures
    assert n_bc >= 64 * (ys.size + 4096) and n_cb >= 64 * (xs.size + 4096) and n_cc >= 8 * (cx.size + 4096)
