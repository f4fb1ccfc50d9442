#!/usr/bin/env python3
"""GPU box: the fused detuned voice (zh_detuned_paint, csrc/detuned.hip) against the same OuterInstrument.paint composed stage by
stage through the existing entry points -- zh_zero, zh_noise_paint, zh_zero, zh_filter_paint, zh_multiply_with_scalar, zh_pow,
zh_multiply_with (a frequency image), zh_zero, zh_trisawosc_paint (frequency image), zh_add_into, zh_multiply_with_scalar, zh_zero,
zh_envelope_paint, zh_zero, zh_multiply, zh_filter_paint: the 16 calls of examples/example_detuned.zig:139-154 and :61-99 -- per
1,024-frame buffer at 4,096 and 131,072 voices, adding into both outputs (ZH_PAINT_ZERO_FIRST off), the reference's patch, a held
note.  Both sides are a graph of K paints on one stream; they alternate A/B in every round; medians and the spread are reported.
Bytes per voice-sample, from the calls' shapes: fused 16 (two read-modify-write columns), composed 140.
usage: tools/detuned_bench.py [rounds]            -> a table on stdout
       tools/detuned_bench.py --profile VOICES    -> a few fused paints and nothing else (for a counter run of rocprofv3)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import abi, modules as mod, zang
from zang_amd.runtime import image_row_pad

PROFILE = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--profile" else 0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and not PROFILE else 9
F, SR, K, FREQ, SEED = 1024, 48000.0, 10, 220.0, 0
PATCH = mod.Detuned.Patch()
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)


def fused(V):
    m = mod.Detuned(V, ctx, SEED)
    p = m.Params(SR, FREQ, True, 0, PATCH)
    return [m], lambda out, sync: m.paint(span, [out, sync], None, False, p)


def composed(V):
    """OuterInstrument.paint over Instrument.paint, call by call"""
    noise, nf, osc, env, mf = mod.Noise(V, ctx, SEED), mod.Filter(V, ctx), mod.TriSawOsc(V, ctx), mod.Envelope(V, ctx), mod.Filter(V, ctx)
    dev = torch.device(ctx.device)
    W = V + image_row_pad(V)                                                                    # rows padded as ctx.image pads them
    s0, s1, t2, t3 = (torch.zeros((F, W), dtype=torch.float32, device=dev) for _ in range(4))
    two = torch.full((F, W), 2.0, dtype=torch.float32, device=dev)                              # zh_pow walks whole rows, padding included
    freq = torch.full((F, W), FREQ, dtype=torch.float32, device=dev)[:, :V]
    t0, t1, t2, t3 = s0[:, :V], s1[:, :V], t2[:, :V], t3[:, :V]
    cuts = mod.Filter.cutoffFromFrequency(torch.tensor([PATCH.warble_hz, PATCH.cutoff_hz], dtype=torch.float32, device=dev), SR, ctx)
    ctx.sync()
    cut_w, cut_m = (float(x) for x in cuts.cpu())
    cubed = zang.PaintCurve.cubed
    ep = env.Params(SR, cubed(PATCH.attack), cubed(PATCH.decay), cubed(PATCH.release), PATCH.sustain_volume, True)

    def paint(out, sync):
        zang.zero(span, t1, ctx=ctx)                                                            # :139-140
        noise.paint(span, [t1], [], False, noise.Params(mod.Noise.white))
        zang.zero(span, t0, ctx=ctx)                                                            # :141-150
        nf.paint(span, [t0], [], False, nf.Params(t1, mod.Filter.low_pass, zang.constant(cut_w), zang.constant(0.0)))
        zang.multiplyWithScalar(span, t0, PATCH.warble_wide, ctx=ctx)                           # :152-154 (mode 0)
        abi.check(ctx.lib.zh_pow(ctx.handle, F * W, s1.data_ptr(), two.data_ptr(), s0.data_ptr()), "zh_pow")   # :61-65
        zang.multiplyWith(span, t1, freq, ctx=ctx)
        zang.zero(span, t2, ctx=ctx)                                                            # :67-72
        osc.paint(span, [t2], [], False, osc.Params(SR, zang.buffer(t1), PATCH.color))
        zang.addInto(span, sync, t1, ctx=ctx)                                                   # :74
        zang.multiplyWithScalar(span, t2, PATCH.volume, ctx=ctx)                                # :76
        zang.zero(span, t1, ctx=ctx)                                                            # :78-86
        env.paint(span, [t1], [], False, ep)
        zang.zero(span, t3, ctx=ctx)                                                            # :87-88
        zang.multiply(span, t3, t2, t1, ctx=ctx)
        mf.paint(span, [out], [], False, mf.Params(t3, mod.Filter.low_pass, zang.constant(cut_m), zang.constant(PATCH.res)))   # :90-99
    return [noise, nf, osc, env, mf], paint


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
    for _ in range(3):
        paint(out, sync)
    ctx.sync()
    print("3 zh_detuned_paint of %d voices x %d frames (k_detuned): expect 2 x 2 x %d bytes read and written per paint" % (PROFILE, F, PROFILE * F * 4))
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
    a_paint(same[0], same[1]); b_paint(same[2], same[3]); ctx.sync()
    assert torch.equal(same[0].view(torch.int32), same[2].view(torch.int32)) and torch.equal(same[1].view(torch.int32), same[3].view(torch.int32)), "the two forms differ"
    assert float(same[0].abs().max()) > 0.001 and float(same[1].min()) > 100.0, "silence"
    del same
    cases = [("fused: zh_detuned_paint (k_detuned)", graph_of(a_paint, outs, syncs)),
             ("composed: 16 calls through existing entry points", graph_of(b_paint, outs, syncs))]
    for _, g in cases:
        timed(g)
    times = {name: [] for name, _ in cases}
    for r in range(ROUNDS):
        for name, g in (cases if r % 2 == 0 else cases[::-1]):
            times[name].append(timed(g))
    med = {name: statistics.median(times[name]) for name, _ in cases}
    for name, g in cases:
        print("%-10d %-50s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, name, med[name], min(times[name]), max(times[name]), med[name] / med[cases[0][0]],
                                                                 V * F / (med[name] * 1e-6)))
        g.close()
    for m in a_mods + b_mods:
        m.close()
    del outs, syncs, cases
