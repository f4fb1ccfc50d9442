#!/usr/bin/env python3
"""GPU box: the fused lead voices (zh_porta_paint_spans, zh_vibrato_paint_spans; csrc/lead.hip k_lead_spans) against the same
sub-spans composed stage by stage through the entry points that existed before them:
  portamento  zh_zero, zh_portamento_paint, zh_zero, zh_envelope_paint, zh_zero, zh_sineosc_paint (frequency image), zh_multiply,
              zh_add_into: the 8 calls of examples/example_portamento.zig:53-85, prev_note_on carried by the caller;
  vibrato     zh_zero, zh_sineosc_paint, zh_multiply_with_scalar, zh_add_scalar_into, zh_multiply_with_scalar (the three roundings
              of :54), zh_add_into, zh_zero, zh_pulseosc_paint (frequency image), zh_zero, zh_gate_paint, zh_multiply: 11 calls,
              examples/example_vibrato.zig:46-67
per 1,024-frame buffer at 4,096 and 131,072 voices, adding into both outputs (ZH_PAINT_ZERO_FIRST off), the reference's patches.
The sub-spans: ONE per voice, the whole buffer, a held note (note_on set, note_id_changed clear, prev_note_on set) -- the table a
live player's bank writes between key events, and the one shape the plain paints of the earlier entry points can restate (the
Portamento has no span paint).  Both sides are a graph of K paints on one stream; they alternate A/B in every round; medians and
the spread are reported.  Bytes per voice-sample, from the calls' shapes: fused 16 (two read-modify-write columns), composed 68
(portamento) and 92 (vibrato).
usage: tools/lead_bench.py [rounds] [--out FILE]   -> a table on stdout and in FILE (default profiles/r17/lead_bench.txt)"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import modules as mod, zang

args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "r17", "lead_bench.txt")
if "--out" in args:
    i = args.index("--out")
    OUT = args[i + 1]
    del args[i:i + 2]
ROUNDS = int(args[0]) if args else 9
F, SR, K, FREQ = 1024, 48000.0, 10, 220.0
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def one_span_table(m, V, nic):
    full = lambda x, dt: np.full((1, V), x, dt)
    tab = m.span_table(np.ones(V, np.uint32), full(0, np.uint32), full(F, np.uint32), full(nic, np.uint8),
                       {"freq": (full(FREQ, np.float32), None), "note_on": (None, full(1, np.uint32))})
    tab.device(ctx.device, ["freq", "note_on"])          # uploaded before a capture records
    return tab


def fused(cls, V):
    m = cls(V, ctx)
    p = m.Params(SR, 0.0, False)                         # both fields come from the span arrays
    tabs = {True: one_span_table(m, V, 1), False: one_span_table(m, V, 0)}
    return [m], lambda out, sync, first=False: m.paint_spans(span, [out, sync], None, p, tabs[first])


def temps_of(V):
    return [ctx.image(F, V, fill=0.0) for _ in range(3)]


def composed_porta(V):
    """Instrument.paint of example_portamento.zig, call by call; first = the note's first buffer (prev_note_on clear)"""
    P = mod.Porta.Patch()
    porta, env, osc = mod.Portamento(V, ctx), mod.Envelope(V, ctx), mod.SineOsc(V, ctx)
    t0, t1, t2 = temps_of(V)
    cubed = zang.PaintCurve.cubed
    ep = env.Params(SR, cubed(P.attack), cubed(P.decay), cubed(P.release), P.sustain_volume, True)

    def paint(out, sync, first=False):
        zang.zero(span, t0, ctx=ctx)                                                            # :53-61
        porta.paint(span, [t0], [], first, porta.Params(SR, cubed(P.glide), FREQ, True, not first))
        zang.zero(span, t1, ctx=ctx)                                                            # :63-73
        env.paint(span, [t1], [], first, ep)
        zang.zero(span, t2, ctx=ctx)                                                            # :75-80
        osc.paint(span, [t2], [], False, osc.Params(SR, zang.buffer(t0), zang.constant(0.0)))
        zang.multiply(span, out, t1, t2, ctx=ctx)                                               # :82
        zang.addInto(span, sync, t0, ctx=ctx)                                                   # :85
    return [porta, env, osc], paint


def composed_vibrato(V):
    """Instrument.paint of example_vibrato.zig, call by call"""
    P = mod.Vibrato.Patch()
    vib, osc, gate = mod.SineOsc(V, ctx), mod.PulseOsc(V, ctx), mod.Gate(V, ctx)
    t0, t1, t2 = temps_of(V)

    def paint(out, sync, first=False):
        zang.zero(span, t2, ctx=ctx)                                                            # :46-51
        vib.paint(span, [t2], [], False, vib.Params(SR, zang.constant(P.vib_hz), zang.constant(0.0)))
        zang.multiplyWithScalar(span, t2, P.depth, ctx=ctx)                                     # :52-55, one rounding per call
        zang.addScalarInto(span, t2, 1.0, ctx=ctx)
        zang.multiplyWithScalar(span, t2, FREQ, ctx=ctx)
        zang.addInto(span, sync, t2, ctx=ctx)                                                   # :56
        zang.zero(span, t0, ctx=ctx)                                                            # :57-62
        osc.paint(span, [t0], [], False, osc.Params(SR, zang.buffer(t2), P.color))
        zang.zero(span, t1, ctx=ctx)                                                            # :63-66
        gate.paint(span, [t1], [], False, gate.Params(True))
        zang.multiply(span, out, t0, t1, ctx=ctx)                                               # :67
    return [vib, osc, gate], paint


def graph_of(paint, outs, syncs):
    """K paints into rings of output images as one graph"""
    for i in range(2):
        paint(outs[i % len(outs)], syncs[i % len(syncs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)], syncs[i % len(syncs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


say("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min - max)" % (F, K, ROUNDS))
say("%-10s %-58s %26s %8s %16s" % ("voices", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096, 131072):
    for name, cls, composed, calls in (("porta", mod.Porta, composed_porta, 8), ("vibrato", mod.Vibrato, composed_vibrato, 11)):
        nout = max(2, min(16, (128 << 20) // (F * V * 4)))   # two rings of 128 MiB: an image is not still in a cache at the next paint
        outs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
        syncs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
        a_mods, a_paint = fused(cls, V)
        b_mods, b_paint = composed(V)
        same = [ctx.image(F, V, fill=0.0) for _ in range(4)]
        for first in (True, False):                          # the note's first buffer, then a held one: the state carries
            a_paint(same[0], same[1], first); b_paint(same[2], same[3], first)
        ctx.sync()
        assert torch.equal(same[0].view(torch.int32), same[2].view(torch.int32)) and torch.equal(same[1].view(torch.int32), same[3].view(torch.int32)), "the two forms differ"
        assert float(same[0].abs().max()) > 0.001 and float(same[1].min()) > 100.0, "silence"
        del same
        cases = [("fused: zh_%s_paint_spans (k_lead_spans)" % name, graph_of(a_paint, outs, syncs)),
                 ("composed: %d calls through earlier entry points" % calls, graph_of(b_paint, outs, syncs))]
        for _, g in cases:
            timed(g)
        times = {n: [] for n, _ in cases}
        for r in range(ROUNDS):
            for n, g in (cases if r % 2 == 0 else cases[::-1]):
                times[n].append(timed(g))
        med = {n: statistics.median(times[n]) for n, _ in cases}
        for n, g in cases:
            say("%-10d %-58s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, name + " " + n, med[n], min(times[n]), max(times[n]), med[n] / med[cases[0][0]],
                                                                     V * F / (med[n] * 1e-6)))
            g.close()
        for m in a_mods + b_mods:
            m.close()
        del outs, syncs, cases
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
