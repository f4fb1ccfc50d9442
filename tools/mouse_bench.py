#!/usr/bin/env python3
"""GPU box: one buffer of the mouse example's voice fused (zh_pmctl_paint_controlled; csrc/pmctl.hip k_pmctl_controlled) against
the composition a caller has without it on the same streams: per control zh_zero of its image and one zh_portamento_paint per row
(the library has no Portamento span paint: the rows' boundaries are the same for every player here, values per player), then
zh_pmctl_paint_spans with the two images as buffers.
Per 1,024-frame buffer at 4,096 players, zero-first into the output, four rows per stream: the controls at 0 / 256 / 512 / 768, the
notes at 0 / 300 / 600 / 900 (on, on, off, on).  Every side is a graph of K paints on one stream; they alternate in every round;
medians and the spread are reported.  Bytes per voice-sample, from the calls' shapes: fused 4 (the output's store) or, with the
carried temp image, 12 (+ its load and store); composed 36 or 44 in eleven launches -- 4 + 4 the two zeroes, 8 + 8 the Portamentos'
read-modify-writes, 8 the voice's two reads, 4 the output, + 8 the temp.
usage: tools/mouse_bench.py [rounds] [--out FILE]   -> a table on stdout and in FILE (default profiles/r23/mouse_bench.txt)"""
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
OUT = os.path.join(ROOT, "profiles", "r23", "mouse_bench.txt")
if "--out" in args:
    i = args.index("--out")
    OUT = args[i + 1]
    del args[i:i + 2]
ROUNDS = int(args[0]) if args else 9
F, SR, K = 1024, 48000.0, 10
CTL = [0, 256, 512, 768, F]
NOTES = [(0, 300, 1), (300, 600, 1), (600, 900, 0), (900, F, 1)]
SCALES = (4.0, 2.0)
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
span = zang.Span(0, F)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def streams(V):
    """-> (notes table, [ratio, multiplier] as host dicts)"""
    rng = np.random.default_rng(V)
    rows = len(NOTES)
    start = np.repeat(np.array([s for s, _, _ in NOTES], np.uint32)[:, None], V, 1)
    end = np.repeat(np.array([e for _, e, _ in NOTES], np.uint32)[:, None], V, 1)
    on = np.repeat(np.array([o for _, _, o in NOTES], np.uint32)[:, None], V, 1)
    nic = (on != 0).astype(np.uint8)
    nic[1] = 0
    notes = mod.PMCtl.span_table(np.full(V, rows, np.uint32), start, end, nic,
                                 {"freq": (rng.uniform(110.0, 880.0, (rows, V)).astype(np.float32), None), "note_on": (None, on)})
    ctls = []
    for _ in range(2):
        n = len(CTL) - 1
        ctls.append({"count": np.full(V, n, np.uint32), "start": np.repeat(np.array(CTL[:-1], np.uint32)[:, None], V, 1),
                     "end": np.repeat(np.array(CTL[1:], np.uint32)[:, None], V, 1), "nic": np.ones((n, V), np.uint8),
                     "value": rng.uniform(0.0, 1.0, (n, V)).astype(np.float32), "note_on": np.ones((n, V), np.uint32)})
    return notes, ctls


def fused(V, notes, ctls, temp):
    m = mod.PMCtl(V, ctx)
    p = m.Params(SR, relative=True)
    controls = [m.Control(m.control_table(c["count"], c["start"], c["end"], c["nic"], c["value"], c["note_on"]), s) for c, s in zip(ctls, SCALES)]
    stale = [None, ctx.image(F, V, fill=0.0), None] if temp else None
    return [m], lambda out: m.paint_controlled(span, [out], stale, p, notes, controls[0], controls[1], zero_first=True)


def composed(V, notes, ctls, temp):
    m, portas = mod.PMCtl(V, ctx), [mod.Portamento(V, ctx) for _ in range(2)]
    p = m.Params(SR, relative=True)
    imgs = [ctx.image(F, V, fill=0.0) for _ in range(2)]
    stale = [None, ctx.image(F, V, fill=0.0), None] if temp else None
    curve = zang.PaintCurve.linear(0.1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    rows = []
    for c, s in zip(ctls, SCALES):
        rows.append([(zang.Span(int(c["start"][k, 0]), int(c["end"][k, 0])), dev(c["nic"][k]),
                      portas[0].Params(SR, curve, dev((c["value"][k] * np.float32(s)).astype(np.float32)), dev(c["note_on"][k].astype(np.uint8)), True))
                     for k in range(int(c["count"][0]))])
    cobs = [zang.buffer(i) for i in imgs]

    def paint(out):                                                                             # example_mouse.zig:148-211
        for img, porta, rr in zip(imgs, portas, rows):
            zang.zero(span, img, ctx)
            for sp, nic, pp in rr:
                porta.paint(sp, [img], [], nic, pp)
        m.paint_spans(span, [out], stale, p, notes, cobs[0], cobs[1], zero_first=True)
    return [m] + portas, paint


def graph_of(paint, outs):
    """K paints into a ring of output images as one graph"""
    for i in range(2):
        paint(outs[i % len(outs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


say("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min - max)" % (F, K, ROUNDS))
say("%-8s %-100s %26s %8s %16s" % ("players", "form", "us/paint", "ratio", "voice-samples/s"))
for V in (4096,):
    nout = max(2, min(16, (128 << 20) // (F * V * 4)))   # a ring of 128 MiB: an image is not still in a cache at the next paint
    outs = [ctx.image(F, V, fill=0.0) for _ in range(nout)]
    notes, ctls = streams(V)
    sides = [("fused: zh_pmctl_paint_controlled (k_pmctl_controlled), carried temp image", fused(V, notes, ctls, True)),
             ("fused, no temp image", fused(V, notes, ctls, False)),
             ("composed: (zh_zero, zh_portamento_paint x 4) x 2, zh_pmctl_paint_spans with buffers; carried temp image", composed(V, notes, ctls, True))]
    same = [ctx.image(F, V, fill=0.0) for _ in range(2)]
    for _ in range(2):                                   # twice: the state and the temp carry
        sides[0][1][1](same[0]); sides[2][1][1](same[1])
    ctx.sync()
    assert torch.equal(same[0].view(torch.int32), same[1].view(torch.int32)), "the two forms differ"
    assert float(same[0].abs().max()) > 0.1, "silence"
    del same
    cases = [(n, graph_of(paint, outs)) for n, (_, paint) in sides]
    for n, g in cases:
        say("# %s: %s" % (n.split(":")[0].split(",")[0] + (" (no temp)" if "no temp" in n else ""), ", ".join("%s x%d" % kv for kv in g.kernels())))
        timed(g)
    times = {n: [] for n, _ in cases}
    for r in range(ROUNDS):
        for n, g in (cases if r % 2 == 0 else cases[::-1]):
            times[n].append(timed(g))
    med = {n: statistics.median(times[n]) for n, _ in cases}
    for n, g in cases:
        say("%-8d %-100s %9.1f (%6.1f - %6.1f) %8.2f %16.3e" % (V, n, med[n], min(times[n]), max(times[n]), med[n] / med[cases[0][0]], V * F / (med[n] * 1e-6)))
        g.close()
    for mods, _ in (s for _, s in sides):
        for m in mods:
            m.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
