#!/usr/bin/env python3
"""StereoEchoes(15000) on one GPU (lines for profiles/rNN/stereo_echoes.txt), 1,024 frames per paint, HIP events around runs of
paints, the routes alternating in one process after a warm-up:

  1. fused: zh_stereo_echoes_paint, against the six-call composition of the same library (addInto x2, SimpleDelay zero-first,
     FilteredEchoes zero-first, addInto, SimpleDelay `+=`) on the same images, at 4,096 and 131,072 voices.  Both are `+=` paints
     (the composition has no zero-first form); the fused paint with ZH_PAINT_ZERO_FIRST is timed beside them.
     The bar: the fused median below the composition's fastest round, at both sizes.
  2. crossover: the role-wave form (k_stereo_echoes_pc) against the lane-per-voice walk (stereo_echoes_pc_max = 0), zero-first, at voice
     counts from 1,024 to 131,072.
  3. SongBank: N songs x `--seconds` of song with and without echoes (host clock around render(), which ends in the copy to the
     host); times only.

    python tools/stereo_echoes_bench.py [--rounds 7] [--only fused|crossover|bank] [--songs 1024] [--seconds 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

os.environ["ZH_ENV_LIVE"] = "1"                      # ZH_FORMS is read again at every paint (the crossover flips a row)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, MAIN = 1024, 15000
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(torch, fn, reps):
    """microseconds per call of fn() between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def bench_fused(ctx, rounds, V):
    import torch
    from zang_amd import modules as mod, zang
    sp = zang.Span(0, F)
    inp, L, R, g0, g1 = (ctx.image(F, V) for _ in range(5))
    inp.uniform_(-1.0, 1.0)
    fused = mod.StereoEchoes(V, MAIN, ctx)
    d0, d1, fe = mod.SimpleDelay(V, MAIN // 2, ctx), mod.SimpleDelay(V, MAIN // 2, ctx), mod.FilteredEchoes(V, MAIN, ctx)
    P = fused.Params(inp, 0.6, 0.1)

    def a_fused():
        fused.paint(sp, [L, R], None, False, P)

    def a_fused_zf():
        fused.paint(sp, [L, R], None, False, P, zero_first=True)

    def b_composition():
        zang.addInto(sp, L, inp, ctx=ctx); zang.addInto(sp, R, inp, ctx=ctx)
        d0.paint(sp, [g0], [], False, d0.Params(inp), zero_first=True)
        fe.paint(sp, [g1], None, False, fe.Params(g0, 0.6, 0.1), zero_first=True)
        zang.addInto(sp, L, g1, ctx=ctx)
        d1.paint(sp, [R], [], False, d1.Params(g1))
    # the two routes give the same bits from the same state
    L.zero_(); R.zero_(); a_fused(); ctx.sync()
    wantL, wantR = L.clone(), R.clone()
    L.zero_(); R.zero_(); b_composition(); ctx.sync()
    assert torch.equal(L.view(torch.int32), wantL.view(torch.int32)) and torch.equal(R.view(torch.int32), wantR.view(torch.int32)), "fused and composition differ"
    del wantL, wantR
    a_fused(); kernel = ctx.last_form()
    reps = 20 if V <= 16384 else 5
    for fn in (a_fused, a_fused_zf, b_composition):                  # warm-up of everything timed below
        timed(torch, fn, reps)
    ta, tz, tb = [], [], []
    for _ in range(rounds):
        L.zero_(); R.zero_()                                         # (`+=` paints: keep the sums finite)
        ta.append(timed(torch, a_fused, reps))
        tb.append(timed(torch, b_composition, reps))
        tz.append(timed(torch, a_fused_zf, reps))
    (ma, la, ha), (mz, lz, hz), (mb, lb, hb) = stats(ta), stats(tz), stats(tb)
    say(f"fused: StereoEchoes({MAIN}), {V} voices x {F} frames, kernel {', '.join(kernel)}, {rounds} alternating rounds of {reps} paints")
    say(f"fused:   one kernel, `+=`:      {ma:8.1f} us (min {la:.1f}, max {ha:.1f}) = {44 * V * F / ma / 1e6:.2f} TB/s of its 44 B per voice-sample")
    say(f"fused:   one kernel, zero-first: {mz:8.1f} us (min {lz:.1f}, max {hz:.1f}) = {36 * V * F / mz / 1e6:.2f} TB/s of its 36 B per voice-sample")
    say(f"fused:   six-call composition:  {mb:8.1f} us (min {lb:.1f}, max {hb:.1f}) = {88 * V * F / mb / 1e6:.2f} TB/s of its 88 B per voice-sample")
    ok = ma < lb
    say(f"fused:   fused median {ma:.1f} us against the composition's fastest round {lb:.1f} us: {mb / ma:.2f} x at the medians, "
        f"{'below' if ok else 'NOT below'}")
    for m in (fused, d0, d1, fe):
        m.close()
    return ok


def bench_crossover(ctx, rounds, counts):
    import torch
    from zang_amd import modules as mod, zang
    sp = zang.Span(0, F)
    say(f"crossover: StereoEchoes({MAIN}), zero-first, {F} frames: role waves (k_stereo_echoes_pc) against the walk (stereo_echoes_pc_max=0), {rounds} alternating rounds")
    for V in counts:
        inp, L, R = (ctx.image(F, V) for _ in range(3))
        inp.uniform_(-1.0, 1.0)
        m = mod.StereoEchoes(V, MAIN, ctx)
        P = m.Params(inp, 0.6, 0.1)
        paint = lambda: m.paint(sp, [L, R], None, False, P, zero_first=True)
        reps = 20 if V <= 16384 else 5
        t = {"pc": [], "walk": []}
        names = {}
        for r in range(rounds + 1):                                  # round 0 warms up
            for form, env in (("pc", "stereo_echoes_pc_max=4294967295"), ("walk", "stereo_echoes_pc_max=0")):
                os.environ["ZH_FORMS"] = env
                x = timed(torch, paint, reps)
                names[form] = ", ".join(ctx.last_form())
                if r:
                    t[form].append(x)
        os.environ.pop("ZH_FORMS", None)
        (mp, lp, hp), (mw, lw, hw) = stats(t["pc"]), stats(t["walk"])
        say(f"crossover: {V:7d} voices: {names['pc']} {mp:8.1f} us (min {lp:.1f}, max {hp:.1f}); {names['walk']} {mw:8.1f} us (min {lw:.1f}, max {hw:.1f}); "
            f"role waves / walk = {mp / mw:.2f}")
        m.close()
        del inp, L, R


def bench_bank(ctx, rounds, seconds, n, text):
    import torch
    from zang_amd import song, songbank
    base = song.resolve_frequencies(song.compile_song(text), ctx)
    banks = {"dry, mono": songbank.SongBank(ctx, [base] * n), "echoes, stereo": songbank.SongBank(ctx, [base] * n, echoes=(MAIN, 0.6, 0.1))}
    t = {k: [] for k in banks}
    for r in range(rounds + 1):                                      # round 0 warms up
        for k, b in banks.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.render(seconds)
            if r:
                t[k].append(time.perf_counter() - t0)
    say(f"bank: SongBank N = {n}, {seconds:g} s of song per render, {rounds} alternating rounds after a warm-up render")
    for k in banks:
        m, lo, hi = stats(t[k])
        say(f"bank:   {k}: {m:.3f} s (min {lo:.3f}, max {hi:.3f})")
    b = banks["echoes, stereo"]
    b.trace_kernels = True
    b.render_batch([F] * 8)
    b.trace_kernels = False
    say(f"bank:   kernels of one batch of 8 buffers with echoes: {', '.join(b.last_kernels)}; overflows {b.overflows()}")
    for b in banks.values():
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["fused", "crossover", "bank"])
    ap.add_argument("--voices", default="4096,131072")
    ap.add_argument("--crossover", default="1024,4096,16384,32768,65536,131072")
    ap.add_argument("--songs", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--song", default=os.path.join(ROOT, "tests", "golden", "example_song.txt"))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stereo_echoes_bench: no GPU; nothing is measured without one")
    import zang_amd
    ctx = zang_amd.default_context()
    say(f"device: {torch.cuda.get_device_name(0)}")
    ok = True
    if a.only in (None, "fused"):
        for V in [int(x) for x in a.voices.split(",")]:
            ok = bench_fused(ctx, a.rounds, V) and ok
    if a.only in (None, "crossover"):
        bench_crossover(ctx, a.rounds, [int(x) for x in a.crossover.split(",")])
    if a.only in (None, "bank"):
        bench_bank(ctx, max(3, a.rounds // 2), a.seconds, a.songs, open(a.song).read())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(LINES) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
