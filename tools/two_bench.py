#!/usr/bin/env python3
"""GPU box: the fused voice of the two-source example (zh_dual_paint_spans; csrc/dual.hip k_dual_spans) against what a caller had
before it for the same merged table, the composition the reference performs through the builtin span paints and the basics:
zh_zero, zh_trisawosc_paint_spans, zh_zero, zh_envelope_paint_spans over two temp images, zh_multiply into the output and one
zh_add_scalar_into per sub-span into the frequency image -- and the merge stage's launch (zh_span_merge_schedule, k_span_merge)
alone.  Both sides read the stage's own table in place.
Per 1,024-frame buffer at 4,096 and 131,072 voices, adding into both outputs.  The sources, the same in every player: A = {220 Hz,
on} over [0, 500) and {330 Hz, on} over [500, 1024); B = {0.5, off} over [0, 300) and {0.853, on} over [300, 1024); merged: THREE
sub-spans per voice.  Both sides are a graph of K paints on one stream; they alternate A/B in every round; medians and the spread
are reported.  Bytes per voice-sample, from the calls' shapes: fused 16 (two read-modify-write columns); composed 48 in seven
launches -- 4 + 4 the two zeroes, 8 + 8 the two modules' read-modify-writes of their temps, 16 the multiply, 8 the scalar adds.
usage: tools/two_bench.py [rounds] [--out FILE]   -> a table on stdout and in FILE (default profiles/r21/two_bench.txt)"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import modules as mod, two, zang
from zang_amd.bank import LiveVoiceBank

args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "r21", "two_bench.txt")
if "--out" in args:
    i = args.index("--out")
    OUT = args[i + 1]
    del args[i:i + 2]
ROUNDS = int(args[0]) if args else 9
F, SR, K = 1024, 48000.0, 10
SRC_A = [(0, 220.0, 1), (500, 330.0, 1)]                 # (frame, freq, note_on)
SRC_B = [(0, 0.5, 0), (300, 0.853, 1)]                   # (frame, color, note_on)
SYNC = [(0, 500, 220.0), (500, F, 330.0)]                # what :109 adds, per source-A sub-span
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def merged(V):
    """two live banks of polyphony 1 scheduled once, and the stage over their tables: -> (objects, run the stage, its table)"""
    banks = []
    for dtype, name, src in ((two.FREQ_PARAMS, "freq", SRC_A), (two.COLOR_PARAMS, "color", SRC_B)):
        bank = LiveVoiceBank(ctx, V, 1, dtype, dtype.fields["on"][1], len(src) * V, rows=two.SOURCE_SPANS)
        for k, (frame, value, on) in enumerate(src):
            rec = np.zeros(V, dtype)
            rec[name], rec["note_on"], rec["on"] = value, on, 1
            bank.push(np.arange(V, dtype=np.uint32), np.full(V, frame, np.uint32), np.full(V, k + 1, np.uint64), rec)
        bank.schedule(F, two.SOURCE_SPANS)
        banks.append((bank, bank.script_table(two.SOURCE_SPANS, {name: (0, "f"), "note_on": (1, "u")})))
    stage = two.SpanMerge(ctx, V, [("freq", "f"), ("note_on_a", "u")], "note_on_a", [("color", "f"), ("note_on_b", "u")], "note_on_b")
    run = lambda: stage.schedule(F, two.MAX_SPANS, banks[0][1], ("freq", "note_on"), banks[1][1], ("color", "note_on"))
    run(); ctx.sync()
    assert stage.download(two.MAX_SPANS)["count"].tolist() == [3] * V and stage.overflows() == 0
    return [b for b, _ in banks] + [stage], run, stage.script_table(two.MAX_SPANS)


def fused(V, tab):
    m = mod.Dual(V, ctx)
    p = m.Params(SR, 0.0, 0.0, False)
    return [m], lambda out, sync: m.paint_spans(span, [out, sync], None, p, tab)


def composed(V, tab):
    tri, env = mod.TriSawOsc(V, ctx), mod.Envelope(V, ctx)
    t0, t1 = ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)
    pt = tri.Params(SR, zang.constant(0.0), 0.0)
    cubed = zang.PaintCurve.cubed
    pe = env.Params(SR, cubed(0.025), cubed(0.1), cubed(1.0), 0.5, False)

    def paint(out, sync):                                                                       # example_two.zig:83-153
        zang.zero(span, t0, ctx)
        zang.zero(span, t1, ctx)
        for s, e, freq in SYNC:
            zang.addScalarInto(zang.Span(s, e), sync, freq, ctx)
        tri.paint_spans(span, [t0], [], pt, tab)
        env.paint_spans(span, [t1], [], pe, tab)
        zang.multiply(span, out, t0, t1, ctx)
    return [tri, env], paint


def graph_of(paint, outs):
    """K paints into a ring of (output, sync) image pairs as one graph"""
    for i in range(2):
        paint(*outs[i % len(outs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(*outs[i % len(outs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


say("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min - max)" % (F, K, ROUNDS))
say("%-10s %-106s %26s %8s %16s" % ("voices", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096, 131072):
    nout = max(2, min(16, (128 << 20) // (2 * F * V * 4)))   # a ring of 128 MiB: an image is not still in a cache at the next paint
    outs = [(ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)) for _ in range(nout)]
    s_mods, s_run, tab = merged(V)
    a_mods, a_paint = fused(V, tab)
    b_mods, b_paint = composed(V, tab)
    same = [(ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)) for _ in range(2)]
    for _ in range(2):                                   # twice: the state carries
        a_paint(*same[0]); b_paint(*same[1])
    ctx.sync()
    for x, y in zip(same[0], same[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the two forms differ"
    assert float(same[0][0].abs().max()) > 0.1 and float(same[0][1].max()) == 660.0, "silence"
    del same
    cases = [("fused: zh_dual_paint_spans (k_dual_spans)", graph_of(a_paint, outs)),
             ("composed: zh_zero x 2, zh_add_scalar_into x 2, zh_trisawosc_paint_spans, zh_envelope_paint_spans, zh_multiply", graph_of(b_paint, outs))]
    for _, g in cases:
        timed(g)
    times = {n: [] for n, _ in cases}
    for r in range(ROUNDS):
        for n, g in (cases if r % 2 == 0 else cases[::-1]):
            times[n].append(timed(g))
    med = {n: statistics.median(times[n]) for n, _ in cases}
    for n, g in cases:
        say("%-10d %-106s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, n, med[n], min(times[n]), max(times[n]), med[n] / med[cases[0][0]], V * F / (med[n] * 1e-6)))
        g.close()
    sg = ctx.capture(lambda: [s_run() for _ in range(K)])
    timed(sg)
    ts = [timed(sg) for _ in range(ROUNDS)]
    say("%-10d %-106s %9.1f (%6.1f - %6.1f)" % (V, "zh_span_merge_schedule alone (k_span_merge), two sub-spans a source, three merged", statistics.median(ts), min(ts), max(ts)))
    sg.close()
    for m in a_mods + b_mods + s_mods:
        m.close()
    del outs, cases, tab
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
