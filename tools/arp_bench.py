#!/usr/bin/env python3
"""GPU box: the fused HardSquare span paint (zh_hard_square_paint_spans; csrc/hard_square.hip k_hard_square_spans) against what a
caller had before it for the same sub-spans: the zangscript-generated HardSquare module's paint_spans (tests/golden/
script_modules.txt) for the voice, plus one zh_add_scalar_into per sub-span for the frequency image of
examples/example_arpeggiator.zig:115 -- and the arpeggiator stage's launch (zh_arp_schedule, k_arp_schedule) alone.
Per 1,024-frame buffer at 4,096 and 131,072 voices, adding into both outputs.  The sub-spans: TWO per voice, [0, 500) a carried
note and [500, 1024) a new one, the same frames and frequencies in every voice (what the composed side's scalar adds can restate;
at 48 kHz a note lasts 1,440 frames, so a buffer holds one boundary or none).  Both sides are a graph of K paints on one stream;
they alternate A/B in every round; medians and the spread are reported.  Bytes per voice-sample, from the calls' shapes: fused 16
(two read-modify-write columns), composed 16 as well (8 the module, 8 the scalar adds) in three launches.
usage: tools/arp_bench.py [rounds] [--out FILE]   -> a table on stdout and in FILE (default profiles/r18/arp_bench.txt)"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import arp, modules as mod, script, zang
from zang_amd.bank import LiveVoiceBank

args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "r18", "arp_bench.txt")
if "--out" in args:
    i = args.index("--out")
    OUT = args[i + 1]
    del args[i:i + 2]
ROUNDS = int(args[0]) if args else 9
F, SR, K = 1024, 48000.0, 10
SUBS = [(0, 500, 220.0, 0), (500, F, 330.0, 1)]          # (start, end, freq, note_id_changed)
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def arrays(V):
    col = lambda j, dt: np.repeat(np.array([[s[j]] for s in SUBS], dt), V, axis=1)
    return np.full(V, len(SUBS), np.uint32), col(0, np.uint32), col(1, np.uint32), col(3, np.uint8), col(2, np.float32), np.ones((len(SUBS), V), np.uint32)


def fused(V):
    m = mod.HardSquare(V, ctx)
    count, start, end, nic, freq, on = arrays(V)
    tab = m.span_table(count, start, end, nic, {"freq": (freq, None), "note_on": (None, on)})
    tab.device(ctx.device, ["freq", "note_on"])          # uploaded before a capture records
    p = m.Params(SR, 0.0, False)
    return [m], lambda out, sync: m.paint_spans(span, [out, sync], None, p, tab)


def composed(V):
    text = open(os.path.join(ROOT, "tests", "golden", "script_modules.txt")).read()
    prog = script.ScriptProgram(text, ctx, filename="script_modules.txt", only=["HardSquare"], spans=True)
    m = prog.module("HardSquare", V)
    count, start, end, nic, freq, on = arrays(V)
    tab = script.ScriptSpanTable(m.params, count, start, end, nic, {"freq": (freq, None), "note_on": (None, on)})
    params = {"sample_rate": SR, "freq": 0.0, "note_on": False}

    def paint(out, sync):
        m.paint_spans(span, [out], tab, params)
        for s, e, f, _ in SUBS:                                                                 # example_arpeggiator.zig:115
            zang.addScalarInto(zang.Span(s, e), sync, f, ctx=ctx)
    tab.device(ctx.device, [n for n, _, _ in m.params])                                         # uploaded before a capture records
    return [m], paint


def graph_of(paint, outs, syncs):
    """K paints into rings of output images as one graph"""
    for i in range(2):
        paint(outs[i % len(outs)], syncs[i % len(syncs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)], syncs[i % len(syncs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


def stage_graph(V):
    """K launches of the stage over an outer table of one carried sub-span per player (three keys held)"""
    keys = (440.0 * 2.0 ** (np.arange(39) / 12.0)).astype(np.float32)
    bank = LiveVoiceBank(ctx, V, 1, arp.HELD_PARAMS, arp.HELD_PARAMS.fields["on"][1], V, rows=arp.OUTER_SPANS)
    stage = arp.ArpStage(ctx, V, keys, rows=arp.MAX_SPANS)
    rec = np.zeros(V, arp.HELD_PARAMS)
    rec["held_lo"], rec["on"] = 0b10101, 1
    bank.push(np.arange(V, dtype=np.uint32), np.zeros(V, np.uint32), np.ones(V, np.uint64), rec)
    bank.schedule(F, arp.OUTER_SPANS)
    outer = arp.held_table(bank, arp.OUTER_SPANS)
    run = lambda: stage.schedule(SR, F, arp.MAX_SPANS, outer)
    run(); ctx.sync()
    return [bank, stage], ctx.capture(lambda: [run() for _ in range(K)])


say("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min - max)" % (F, K, ROUNDS))
say("%-10s %-72s %26s %8s %16s" % ("voices", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096, 131072):
    nout = max(2, min(16, (128 << 20) // (F * V * 4)))   # two rings of 128 MiB: an image is not still in a cache at the next paint
    outs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    syncs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    a_mods, a_paint = fused(V)
    b_mods, b_paint = composed(V)
    same = [ctx.image(F, V, fill=0.0) for _ in range(4)]
    for _ in range(2):                                   # twice: the state carries
        a_paint(same[0], same[1]); b_paint(same[2], same[3])
    ctx.sync()
    assert torch.equal(same[0].view(torch.int32), same[2].view(torch.int32)) and torch.equal(same[1].view(torch.int32), same[3].view(torch.int32)), "the two forms differ"
    assert float(same[0].abs().max()) > 0.1 and float(same[1].min()) > 100.0, "silence"
    del same
    cases = [("fused: zh_hard_square_paint_spans (k_hard_square_spans)", graph_of(a_paint, outs, syncs)),
             ("composed: script HardSquare paint_spans + %d zh_add_scalar_into" % len(SUBS), graph_of(b_paint, outs, syncs))]
    for _, g in cases:
        timed(g)
    times = {n: [] for n, _ in cases}
    for r in range(ROUNDS):
        for n, g in (cases if r % 2 == 0 else cases[::-1]):
            times[n].append(timed(g))
    med = {n: statistics.median(times[n]) for n, _ in cases}
    for n, g in cases:
        say("%-10d %-72s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, n, med[n], min(times[n]), max(times[n]), med[n] / med[cases[0][0]], V * F / (med[n] * 1e-6)))
        g.close()
    s_mods, sg = stage_graph(V)
    timed(sg)
    ts = [timed(sg) for _ in range(ROUNDS)]
    say("%-10d %-72s %9.1f (%6.1f - %6.1f)" % (V, "zh_arp_schedule alone (k_arp_schedule), one outer sub-span a player", statistics.median(ts), min(ts), max(ts)))
    sg.close()
    for m in a_mods + b_mods + s_mods:
        m.close()
    del outs, syncs, cases
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
