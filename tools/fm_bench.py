#!/usr/bin/env python3
"""GPU box: the fused FM voice (zh_fm_paint, csrc/fm.hip) timed per 1,024-frame buffer at 4,096 and 131,072 voices -- the default
patch and the worst one (modulator feedback 7, waveform 3 on both operators: a dependent chain through up to four sines a frame)
-- beside zh_pmosc_paint, the nearest existing kernel (two sines, one envelope), at the same voice count in alternating rounds;
and zang_amd.fmsynth.FMSynth at 1,024 synths x 8 voices split into its four steps.  The ratio to PMOsc is reported, not gated.
usage: tools/fm_bench.py [rounds]  -> a table on stdout"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zang_amd
from zang_amd import abi, modules as mod, zang, workloads
from zang_amd.fmsynth import FMSynth, MAX_SPANS

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
F, SR, K, GROUP = 1024, 48000.0, 10, 8
torch.cuda.set_stream(torch.cuda.Stream())               # graph capture is not allowed on the default stream
ctx = zang_amd.Context(0)
dev = ctx.device
span = zang.Span(0, F)

DEFAULT = mod.FMInstrument.default_patch()
WORST = list(DEFAULT)
WORST[abi.FM_MOD_FEEDBACK], WORST[abi.FM_MOD_WAVEFORM], WORST[abi.FM_CAR_WAVEFORM] = 7, 3, 3


def lfo_images(n):
    """[F][n] tremolo and vibrato images as FMSynth makes them"""
    out = []
    for hz in (3.7, 6.4):
        m, img = mod.SineOsc(n, ctx), ctx.image(F, n)
        m.paint(span, [img], [], False, m.Params(SR, zang.constant(hz), zang.constant(0.0)), zero_first=True)
        out.append(img)
        m.close()
    return out


def graph_of(paint, outs):
    """K paints into a ring of output images as one graph (state carried from paint to paint)"""
    for i in range(4):
        paint(outs[i % len(outs)])
    ctx.sync()
    return ctx.capture(lambda: [paint(outs[i % len(outs)]) for i in range(K)])


def timed(g):
    t0 = time.perf_counter(); g.launch(); ctx.sync()
    return (time.perf_counter() - t0) * 1e6 / K


print("# %d frames per paint, %d paints per graph launch, %d alternating rounds, one MI355X; us per paint: median (min)" % (F, K, ROUNDS))
print("%-10s %-34s %16s %12s" % ("voices", "kernel", "us/paint", "x PMOsc"))
for V in (4096, 131072):
    freq_h = workloads.voice_params(5, 0, V)[0]
    freq = torch.from_numpy(freq_h).to(dev)
    nout = max(2, min(32, (512 << 20) // (F * V * 4)))   # a ring of 512 MiB: the stores go to HBM, not to a cache that still holds the image
    outs = [ctx.image(F, V) for _ in range(nout)]
    trem, vib = lfo_images(V // GROUP)
    cases = []
    for name, patch in (("FM default patch", DEFAULT), ("FM worst (feedback 7, waveform 3/3)", WORST)):
        m = mod.FMInstrument(V, ctx, group=GROUP)
        m.set_patches(patch)
        cases.append((name, m, graph_of(lambda o, m=m: m.paint(span, [o], None, False, m.Params(SR, trem, vib, freq, True), zero_first=True), outs)))
    rel = torch.full((V,), 0.3, dtype=torch.float32, device=dev)
    pm = mod.PMOscInstrument(V, rel, ctx)
    cases.append(("PMOscInstrument", pm, graph_of(lambda o: pm.paint(span, [o], None, False, pm.Params(SR, freq, True), zero_first=True), outs)))
    for _, _, g in cases:
        timed(g)
    times = {name: [] for name, _, _ in cases}
    for r in range(ROUNDS):
        for name, _, g in (cases if r % 2 == 0 else cases[::-1]):
            times[name].append(timed(g))
    base = statistics.median(times["PMOscInstrument"])
    for name, m, g in cases:
        med = statistics.median(times[name])
        print("%-10d %-34s %8.1f (%6.1f) %12.2f" % (V, name, med, min(times[name]), med / base))
        g.close(); m.close()
    del outs, cases

# ---- FMSynth: 1,024 synths x 8 voices, one buffer = schedule + two LFO paints + the FM span paint + the grouped mixdown
N, P, REPS = 1024, 8, 20
for label, patches in (("default patches (plain image, groups of 8)", None), ("every 4th synth algorithm 0 (split image, groups of 16)", "mixed")):
    if patches == "mixed":
        patches = np.tile(np.array(DEFAULT, np.uint32), (N, 1))
        patches[::4, abi.FM_ALGORITHM] = 0
    s = FMSynth(ctx, N, patches, polyphony=P, sample_rate=SR)
    rng = np.random.default_rng(1)
    for b in range(3):                                   # a few buffers of playing first: six keys down per synth
        for k in range(2):
            s.push(np.arange(N), np.full(N, 100 + 400 * k), np.arange(N) * 0 + 1 + 2 * b + k, rng.uniform(80.0, 1500.0, N), np.ones(N))
        s.paint(F)
    ctx.sync()
    sp = zang.Span(0, F)
    trem, vib, img = s._lfo[0][:F], s._lfo[1][:F], s._image[:F]
    group = P * (2 if s.split else 1)

    def push():
        s.push(np.arange(0, N, 4), np.full(N // 4, 300), np.full(N // 4, 99), np.full(N // 4, 440.0), np.ones(N // 4))

    def schedule():
        push()
        s.bank.schedule(F, MAX_SPANS)

    def lfos():
        for lfo, im, hz in ((s.tremolo_lfo, trem, 3.7), (s.vibrato_lfo, vib, 6.4)):
            lfo.paint(sp, [im], [], False, lfo.Params(SR, zang.constant(hz), zang.constant(0.0)), zero_first=True)
    steps = (("schedule (push 256 impulses + one launch)", schedule), ("LFOs (two SineOsc paints)", lfos),
             ("paint (k_fm_spans)", lambda: s.voices.paint_spans(sp, [img], None, SR, trem, vib, s._table, zero_first=True, split=s.split)),
             ("mixdown (zh_mixdown_groups)", lambda: zang.mixdownGroups(sp, s._mix, img, group, zero_first=True, ctx=ctx)),
             ("whole buffer (256 pushes + FMSynth.paint)", lambda: (push(), s.paint(F))))
    print("# FMSynth %d synths x %d voices, %s: us per buffer, median (min) of %d rounds of %d calls ending in a synchronise" % (N, P, label, ROUNDS, REPS))
    for name, fn in steps:
        fn(); ctx.sync()
        ts = []
        for r in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e6 / REPS)
        print("  %-44s %8.1f (%6.1f)" % (name, statistics.median(ts), min(ts)))
    assert s.overflows() == 0
    s.close()
