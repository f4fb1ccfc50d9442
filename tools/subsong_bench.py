#!/usr/bin/env python3
"""GPU box: the fused inner voice of the subsong example (zh_saw_env_paint_spans; csrc/saw_env.hip k_saw_env_spans) against what a
caller had before it for the same sub-spans, the composition the reference performs through today's entry points: zh_zero,
zh_trisawosc_paint_spans, zh_zero, zh_envelope_paint_spans over two temp images, then zh_multiply into the output -- and the subsong
stage's launch (zh_subsong_schedule, k_subsong_schedule) alone.
Per 1,024-frame buffer at 4,096 and 131,072 voices, adding into the output.  The sub-spans: TWO per voice, [0, 500) a carried note
and [500, 1024) a new one, the same frames in every voice.  Both sides are a graph of K paints on one stream; they alternate A/B in
every round; medians and the spread are reported.  Bytes per voice-sample, from the calls' shapes: fused 8 (one read-modify-write
column); composed 40 in five launches -- 4 + 4 the two zeroes, 8 + 8 the two modules' read-modify-writes of their temps, 16 the
multiply (two reads and a read-modify-write).
usage: tools/subsong_bench.py [rounds] [--out FILE]   -> a table on stdout and in FILE (default profiles/r19/subsong_bench.txt)"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import modules as mod, subsong, zang
from zang_amd.bank import LiveVoiceBank

args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "r19", "subsong_bench.txt")
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
    m = mod.SawEnv(V, ctx)
    count, start, end, nic, freq, on = arrays(V)
    tab = m.span_table(count, start, end, nic, {"freq": (freq, None), "note_on": (None, on)})
    tab.device(ctx.device, ["freq", "note_on"])          # uploaded before a capture records
    p = m.Params(SR, 0.0, False)
    return [m], lambda out: m.paint_spans(span, [out], None, p, tab)


def composed(V):
    tri, env = mod.TriSawOsc(V, ctx), mod.Envelope(V, ctx)
    t0, t1 = ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)
    count, start, end, nic, freq, on = arrays(V)
    tt = tri.span_table(count, start, end, nic, {"freq": (freq, None)})
    te = env.span_table(count, start, end, nic, {"note_on": (None, on)})
    tt.device(ctx.device, [n for n, _ in tri._span_fields]); te.device(ctx.device, [n for n, _ in env._span_fields])
    pt = tri.Params(SR, zang.constant(0.0), 0.0)
    cubed = zang.PaintCurve.cubed
    pe = env.Params(SR, cubed(0.025), cubed(0.1), cubed(0.15), 0.5, False)

    def paint(out):                                                                             # example_subsong.zig:51-66
        zang.zero(span, t0, ctx)
        tri.paint_spans(span, [t0], [], pt, tt)
        zang.zero(span, t1, ctx)
        env.paint_spans(span, [t1], [], pe, te)
        zang.multiply(span, out, t0, t1, ctx)
    return [tri, env], paint


def graph_of(paint, outs):
    """K paints into a ring of output images as one graph"""
    for i in range(2):
        paint(outs[i % len(outs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


def stage_graph(V):
    """K launches of the stage over an outer table of one carried sub-span per player (a key held, the reference's melody)"""
    a4 = 440.0
    melody = [(0.1 * i, min(i + 1, 5), a4 * 2.0 ** (s / 12.0), i < 5) for i, s in enumerate((-9, -13, -14, -18, -21, -21))]
    kit = subsong.MelodyKit(ctx, [melody])
    bank = LiveVoiceBank(ctx, V, 1, subsong.KEY_PARAMS, subsong.KEY_PARAMS.fields["note_on"][1], V, rows=subsong.OUTER_SPANS)
    stage = subsong.SubsongStage(ctx, V, kit, rows=subsong.MAX_SPANS)
    rec = np.zeros(V, subsong.KEY_PARAMS)
    rec["freq"], rec["note_on"], rec["melody"] = 440.0, 1, 0
    bank.push(np.arange(V, dtype=np.uint32), np.zeros(V, np.uint32), np.ones(V, np.uint64), rec)
    bank.schedule(F, subsong.OUTER_SPANS)
    outer = subsong.key_table(bank, subsong.OUTER_SPANS)
    run = lambda: stage.schedule(SR, F, subsong.MAX_SPANS, outer)
    run(); ctx.sync()
    return [bank, stage, kit], ctx.capture(lambda: [run() for _ in range(K)])


say("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min - max)" % (F, K, ROUNDS))
say("%-10s %-84s %26s %8s %16s" % ("voices", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096, 131072):
    nout = max(2, min(16, (128 << 20) // (F * V * 4)))   # a ring of 128 MiB: an image is not still in a cache at the next paint
    outs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    a_mods, a_paint = fused(V)
    b_mods, b_paint = composed(V)
    same = [ctx.image(F, V, fill=0.0) for _ in range(2)]
    for _ in range(2):                                   # twice: the state carries
        a_paint(same[0]); b_paint(same[1])
    ctx.sync()
    assert torch.equal(same[0].view(torch.int32), same[1].view(torch.int32)), "the two forms differ"
    assert float(same[0].abs().max()) > 0.1, "silence"
    del same
    cases = [("fused: zh_saw_env_paint_spans (k_saw_env_spans)", graph_of(a_paint, outs)),
             ("composed: zh_zero, zh_trisawosc_paint_spans, zh_zero, zh_envelope_paint_spans, zh_multiply", graph_of(b_paint, outs))]
    for _, g in cases:
        timed(g)
    times = {n: [] for n, _ in cases}
    for r in range(ROUNDS):
        for n, g in (cases if r % 2 == 0 else cases[::-1]):
            times[n].append(timed(g))
    med = {n: statistics.median(times[n]) for n, _ in cases}
    for n, g in cases:
        say("%-10d %-84s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, n, med[n], min(times[n]), max(times[n]), med[n] / med[cases[0][0]], V * F / (med[n] * 1e-6)))
        g.close()
    s_mods, sg = stage_graph(V)
    timed(sg)
    ts = [timed(sg) for _ in range(ROUNDS)]
    say("%-10d %-84s %9.1f (%6.1f - %6.1f)" % (V, "zh_subsong_schedule alone (k_subsong_schedule), one outer sub-span a player", statistics.median(ts), min(ts), max(ts)))
    sg.close()
    for m in a_mods + b_mods + s_mods[:2]:
        m.close()
    s_mods[2].close()
    del outs, cases
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
