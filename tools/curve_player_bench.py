#!/usr/bin/env python3
"""GPU box: the fused curve voice (zh_curve_player_paint with both columns, csrc/curve_player.hip) against the same
CurvePlayer.paint composed stage by stage through the existing entry points -- two zh_curve_module_paint, two zh_sineosc_paint
(frequency image; frequency and phase image), three zh_zero, two zh_multiply_with_scalar, one zh_add_into: the ten calls of
examples/example_curve.zig:65-94 -- per 1,024-frame buffer at 4,096 and 131,072 voices, adding into both outputs
(ZH_PAINT_ZERO_FIRST off), the example's curves; the sound is started once and carried from paint to paint (note_id_changed
clear: the curves run 183 buffers).  Both sides are a graph of K paints; they alternate A/B in every round; medians and ranges
are reported.  Bytes per voice-sample: the fused paint reads and writes both outputs, 16; the ten calls move 84 (zero 4, curve 8,
scale 8, zero 4, sine 12, zero 4, curve 8, scale 8, sine 16, add 12).
usage: tools/curve_player_bench.py [rounds]            -> a table on stdout
       tools/curve_player_bench.py --profile VOICES    -> a few fused paints and nothing else (for a counter run of rocprofv3)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import modules as mod, sfx, zang

PROFILE = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--profile" else 0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and not PROFILE else 9
F, SR, K = 1024, 48000.0, 10
REL_FREQ = 1.5
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)
kit = sfx.SfxKit(ctx, [sfx.curve_example_effect()])


def fused(V):
    m = mod.CurveVoice(V, ctx)
    p = m.Params(kit, SR, REL_FREQ, 0)
    return [m], lambda out, sync, nic=False: m.paint(span, [out, sync], None, nic, p)


def composed(V):
    """CurvePlayer.paint call by call"""
    curves = {n: torch.tensor([[v, t] for t, v in c], dtype=torch.float32).cuda() for n, c in
              (("m", sfx.CURVE_EXAMPLE_MODULATOR), ("c", sfx.CURVE_EXAMPLE_CARRIER))}
    cm, cc = mod.Curve(V, ctx), mod.Curve(V, ctx)
    om, oc = mod.SineOsc(V, ctx), mod.SineOsc(V, ctx)
    t0, t1 = ctx.image(F, V), ctx.image(F, V)

    def paint(out, sync, nic=False):
        zang.zero(span, t0, ctx=ctx)
        cm.paint(span, [t0], [], nic, cm.Params(SR, mod.Curve.smoothstep, curves["m"]))
        zang.multiplyWithScalar(span, t0, REL_FREQ, ctx=ctx)
        zang.zero(span, t1, ctx=ctx)
        om.paint(span, [t1], [], nic, om.Params(SR, zang.buffer(t0), zang.constant(0.0)))
        zang.zero(span, t0, ctx=ctx)
        cc.paint(span, [t0], [], nic, cc.Params(SR, mod.Curve.smoothstep, curves["c"]))
        zang.multiplyWithScalar(span, t0, REL_FREQ, ctx=ctx)
        oc.paint(span, [out], [], nic, oc.Params(SR, zang.buffer(t0), zang.buffer(t1)))
        zang.addInto(span, sync, t0, ctx=ctx)
    return [cm, cc, om, oc], paint


def graph_of(paint, outs, syncs):
    """K paints into rings of output images as one graph"""
    for i in range(2):
        paint(outs[i % len(outs)], syncs[i % len(syncs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)], syncs[i % len(syncs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


if PROFILE:
    mods, paint = fused(PROFILE)
    out, sync = ctx.image(F, PROFILE, fill=0.0), ctx.image(F, PROFILE, fill=0.0)
    paint(out, sync, True)
    for _ in range(2):
        paint(out, sync)
    ctx.sync()
    print("3 zh_curve_player_paint of %d voices x %d frames (k_curve_player_spans): expect 2 x 2 x %d bytes read and written per paint"
          % (PROFILE, F, PROFILE * F * 4))
    sys.exit(0)

print("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min - max)" % (F, K, ROUNDS))
print("%-10s %-50s %26s %8s %16s" % ("voices", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096, 131072):
    nout = max(2, min(16, (128 << 20) // (F * V * 4)))   # two rings of 128 MiB: an image is not still in a cache at the next paint
    outs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    syncs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    a_mods, a_paint = fused(V)
    b_mods, b_paint = composed(V)
    same = [ctx.image(F, V, fill=0.0) for _ in range(4)]
    a_paint(same[0], same[1], True); b_paint(same[2], same[3], True); ctx.sync()                 # the impulse: every voice starts its sound
    assert torch.equal(same[0].view(torch.int32), same[2].view(torch.int32)) and float(same[0].abs().max()) > 0.5, "the two forms differ"
    assert torch.equal(same[1].view(torch.int32), same[3].view(torch.int32)) and float(same[1].min()) > 100.0, "the frequency images differ"
    del same
    cases = [("fused: zh_curve_player_paint (k_curve_player_spans)", graph_of(a_paint, outs, syncs)),
             ("composed: 10 calls through existing entry points", graph_of(b_paint, outs, syncs))]
    for _, g in cases:
        timed(g)
    times = {name: [] for name, _ in cases}
    for r in range(ROUNDS):
        for name, g in (cases if r % 2 == 0 else cases[::-1]):
            times[name].append(timed(g))
    med = {name: statistics.median(times[name]) for name, _ in cases}
    for name, g in cases:
        print("%-10d %-50s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, name, med[name], min(times[name]), max(times[name]),
                                                                 med[name] / med[cases[0][0]], V * F / (med[name] * 1e-6)))
        g.close()
    for m in a_mods + b_mods:
        m.close()
    del outs, syncs, cases
kit.close()
