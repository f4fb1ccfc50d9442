#!/usr/bin/env python3
"""GPU box: the fused sound-effect voice (zh_laser_paint, csrc/laser.hip) against the same LaserPlayer.paint composed stage by
stage through the existing entry points -- three zh_curve_module_paint, two zh_sineosc_paint (frequency image; frequency and phase
image), five zh_zero, three zh_multiply_with_scalar, one zh_multiply: the 14 calls of examples/example_laser.zig:77-115 -- per
1,024-frame buffer at 4,096 and 131,072 voices, adding into the output (ZH_PAINT_ZERO_FIRST off), the reference's effect restarted
by every paint (note_id_changed set).  Both sides are a graph of K paints; they alternate A/B in every round; medians are reported.
usage: tools/laser_bench.py [rounds]            -> a table on stdout
       tools/laser_bench.py --profile VOICES    -> a few fused paints and nothing else (for a counter run of rocprofv3)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zang_amd
from zang_amd import modules as mod, sfx, zang

PROFILE = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--profile" else 0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and not PROFILE else 9
F, SR, K = 1024, 48000.0, 10
FREQ_MUL, CARRIER_MUL, MODULATOR_MUL, MODULATOR_RAD = 1.0, 2.0, 0.5, 0.5        # the player laser (example_laser.zig:168-186)
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)
kit = sfx.SfxKit(ctx, [sfx.default_effect()])
f32 = np.float32


def fused(V):
    m = mod.Laser(V, ctx)
    p = m.Params(kit, SR, FREQ_MUL, CARRIER_MUL, MODULATOR_MUL, MODULATOR_RAD, 0)
    return [m], lambda out: m.paint(span, [out], None, True, p)


def composed(V):
    """LaserPlayer.paint call by call; the curves are the kit's own device nodes"""
    curves = {n: torch.tensor([[v, t] for t, v in c], dtype=torch.float32).cuda() for n, c in
              (("m", sfx.DEFAULT_MODULATOR), ("c", sfx.DEFAULT_CARRIER), ("v", sfx.DEFAULT_VOLUME))}
    cm, cc, cv = (mod.Curve(V, ctx) for _ in range(3))
    om, oc = mod.SineOsc(V, ctx), mod.SineOsc(V, ctx)
    t0, t1, t2 = (ctx.image(F, V) for _ in range(3))
    mul_m, mul_c = float(f32(FREQ_MUL) * f32(MODULATOR_MUL)), float(f32(FREQ_MUL) * f32(CARRIER_MUL))

    def paint(out):
        zang.zero(span, t0, ctx=ctx)
        cm.paint(span, [t0], [], True, cm.Params(SR, mod.Curve.smoothstep, curves["m"]))
        zang.multiplyWithScalar(span, t0, mul_m, ctx=ctx)
        zang.zero(span, t1, ctx=ctx)
        om.paint(span, [t1], [], True, om.Params(SR, zang.buffer(t0), zang.constant(0.0)))
        zang.multiplyWithScalar(span, t1, MODULATOR_RAD, ctx=ctx)
        zang.zero(span, t0, ctx=ctx)
        cc.paint(span, [t0], [], True, cc.Params(SR, mod.Curve.smoothstep, curves["c"]))
        zang.multiplyWithScalar(span, t0, mul_c, ctx=ctx)
        zang.zero(span, t2, ctx=ctx)
        oc.paint(span, [t2], [], True, oc.Params(SR, zang.buffer(t0), zang.buffer(t1)))
        zang.zero(span, t0, ctx=ctx)
        cv.paint(span, [t0], [], True, cv.Params(SR, mod.Curve.smoothstep, curves["v"]))
        zang.multiply(span, out, t0, t2, ctx=ctx)
    return [cm, cc, cv, om, oc], paint


def graph_of(paint, outs):
    """K paints into a ring of output images as one graph"""
    for i in range(2):
        paint(outs[i % len(outs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


if PROFILE:
    mods, paint = fused(PROFILE)
    out = ctx.image(F, PROFILE, fill=0.0)
    for _ in range(3):
        paint(out)
    ctx.sync()
    print("3 zh_laser_paint of %d voices x %d frames (k_laser): expect 2 x %d bytes read and written per paint" % (PROFILE, F, PROFILE * F * 4))
    sys.exit(0)

print("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min)" % (F, K, ROUNDS))
print("%-10s %-44s %18s %12s %16s" % ("voices", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096, 131072):
    nout = max(2, min(16, (256 << 20) // (F * V * 4)))   # a ring of 256 MiB: the image is not still in a cache at the next paint
    outs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    a_mods, a_paint = fused(V)
    b_mods, b_paint = composed(V)
    same = [ctx.image(F, V, fill=0.0) for _ in range(2)]
    a_paint(same[0]); b_paint(same[1]); ctx.sync()
    assert torch.equal(same[0].view(torch.int32), same[1].view(torch.int32)) and float(same[0].abs().max()) > 0.5, "the two forms differ"
    del same
    cases = [("fused: zh_laser_paint (k_laser)", graph_of(a_paint, outs)), ("composed: 14 calls through existing entry points", graph_of(b_paint, outs))]
    for _, g in cases:
        timed(g)
    times = {name: [] for name, _ in cases}
    for r in range(ROUNDS):
        for name, g in (cases if r % 2 == 0 else cases[::-1]):
            times[name].append(timed(g))
    med = {name: statistics.median(times[name]) for name, _ in cases}
    for name, g in cases:
        print("%-10d %-44s %9.1f (%6.1f) %12.2f %16.3e" % (V, name, med[name], min(times[name]), med[name] / med[cases[0][0]], V * F / (med[name] * 1e-6)))
        g.close()
    for m in a_mods + b_mods:
        m.close()
    del outs, cases
kit.close()
