#!/usr/bin/env python3
"""The output half of a voice bank, measured on one GPU (lines for profiles/rNN/song_bank.txt):

  1. zh_mixdown_groups_pcm at 4,096 groups x 8 voices x 1,024 frames: time per call (HIP events over a run of calls) and the read
     rate V * F * 4 B / t -- over FOUR images taken in turn (537 MB: more than the 256 MiB Infinity Cache holds, so every call
     reads from HBM) and over one image (134 MB: it stays on the die);
     and at 64 groups against the route without it, 64 x (zh_mixdown_voices(ZH_MIX_SEQUENTIAL) on a column view + zh_mix_down),
     alternating, medians and spread over the rounds.
  2. SongBank at N = 64 and N = 1,024 over `--seconds` of song (host clock around render(), which ends in the copy to the host)
     against sequential SongRenderer(scheduler="device") renders of 8 songs, alternating; the kernels of one batch as
     zh_last_form names them.

    python tools/song_bank_bench.py [--rounds 7] [--seconds 10] [--only mix|bank] [--songs 64,1024] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = 1024
COPY_RATE = 6.3e12                     # achievable HBM rate of the part, bytes per second
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def timed(torch, fn, reps):
    """milliseconds per call of fn(i), i = 0 .. reps - 1, between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_mix(ctx, rounds):
    import torch
    from zang_amd import zang
    G, P, vol = 4096, 8, 0.25
    V = G * P
    span = zang.Span(0, F)
    imgs = []
    for k in range(4):
        img = ctx.image(F, V)
        img.copy_(torch.rand((F, V), device=ctx.device) * 2 - 1)
        imgs.append(img)
    pcm = torch.zeros((G, F * 2), dtype=torch.uint8, device=ctx.device)
    s16 = zang.AudioFormat.signed16_lsb

    def fused(img, groups):
        zang.mixdownGroupsPcm(span, pcm[:groups], img[:, :groups * P], P, s16, 1, 0, vol, ctx=ctx)
    mix = torch.zeros((64, F), dtype=torch.float32, device=ctx.device)

    def parent(img, groups):
        for g in range(groups):
            zang.mixdownVoices(span, mix[g], img[:, g * P:(g + 1) * P], zero_first=True, sequential=True, ctx=ctx)
            zang.mixDown(pcm[g], mix[g], s16, 1, 0, vol, ctx=ctx)
    # the two routes give the same bytes
    fused(imgs[0], 64)
    want = pcm[:64].clone()
    pcm.zero_()
    parent(imgs[0], 64)
    assert torch.equal(pcm[:64], want), "fused and per-group routes differ"
    for k in range(4):                                               # warm-up of every shape timed below
        fused(imgs[k], G)
    kernel = ctx.last_form()
    ctx.sync()
    hbm, die, new64, old64 = [], [], [], []
    for _ in range(rounds):
        hbm.append(timed(torch, lambda i: fused(imgs[i % 4], G), 40))
        die.append(timed(torch, lambda i: fused(imgs[0], G), 40))
        new64.append(timed(torch, lambda i: fused(imgs[i % 4], 64), 40))
        old64.append(timed(torch, lambda i: parent(imgs[i % 4], 64), 5))
    say(f"mix: zh_mixdown_groups_pcm {G} groups x {P} voices x {F} frames, s16 mono, kernel {', '.join(kernel)}, {rounds} rounds of 40 calls")
    for name, xs in (("four images in turn (HBM)", hbm), ("one image (on the die)", die)):
        m, lo, hi = med_spread(xs)
        rate = V * F * 4 / (m * 1e-3)
        say(f"mix:   {name}: {m * 1e3:.1f} us per call (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); read rate {rate / 1e12:.2f} TB/s = "
            f"{rate / COPY_RATE:.2f} of the 6.3 TB/s copy rate")
    mn, lon, hin = med_spread(new64)
    mo, loo, hio = med_spread(old64)
    say(f"mix: 64 groups: one call {mn * 1e3:.1f} us (min {lon * 1e3:.1f}, max {hin * 1e3:.1f}); 64 x (column mixdown + zh_mix_down) "
        f"{mo * 1e3:.1f} us (min {loo * 1e3:.1f}, max {hio * 1e3:.1f}) = {mo * 1e3 / 64:.2f} us per group; x 4,096 groups = {mo * 64:.1f} ms")
    say(f"mix: 64 groups: slowest round of the one call {hin * 1e3:.1f} us against the fastest of the per-group route {loo * 1e3:.1f} us: "
        f"{'faster in every round' if hin < loo else 'NOT faster by more than the spread'}")
    return hin < loo


def transposed(notes, semis):
    out = copy.deepcopy(notes)
    for inst in out:
        for e in inst:
            e.semis += semis
    return out


def bench_bank(ctx, rounds, seconds, sizes, text):
    from unittest import mock
    import torch
    from zang_amd import song, songbank
    base = song.compile_song(text)
    variants = [song.resolve_frequencies(transposed(base, s - 6), ctx) for s in range(12)]
    singles = []
    for i in range(8):
        with mock.patch.object(song, "compile_song", lambda t, instruments=song.EXAMPLE_SONG_INSTRUMENTS, i=i: copy.deepcopy(variants[i])):
            singles.append(song.SongRenderer("", ctx, scheduler="device"))
    banks = {n: songbank.SongBank(ctx, [variants[i % 12] for i in range(n)]) for n in sizes}

    def run_bank(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = banks[n].render(seconds)
        return time.perf_counter() - t0, out

    def run_singles():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [r.render(seconds) for r in singles]
        return time.perf_counter() - t0, out
    # warm-up (and: the first 8 songs of a bank are the 8 single renders, byte for byte)
    _, one = run_singles()
    for n in sizes:
        _, got = run_bank(n)
        assert got[:8] == one, "bank and single-song payloads differ"
    tb = {n: [] for n in sizes}
    ts = []
    for _ in range(rounds):
        for n in sizes:
            tb[n].append(run_bank(n)[0])
        ts.append(run_singles()[0])
    ms, los, his = med_spread(ts)
    say(f"bank: {seconds:g} s of song per render, {rounds} alternating rounds after a warm-up render (state carries on: later seconds of the song)")
    say(f"bank: 8 sequential SongRenderer(scheduler='device') renders: {ms:.3f} s (min {los:.3f}, max {his:.3f}) = {ms / 8 * 1e3:.1f} ms per song")
    ok = True
    for n in sizes:
        m, lo, hi = med_spread(tb[n])
        say(f"bank: SongBank N = {n}: {m:.3f} s (min {lo:.3f}, max {hi:.3f}) = {m / n * 1e3:.2f} ms per song, {n * seconds / m:.0f} songs x real time; "
            f"{n} x the per-song time = {ms / 8 * n:.3f} s ({ms / 8 * n / m:.1f} x)")
        if n == 64:
            ok = hi < los / 8 * 64
            say(f"bank: N = 64: slowest round {hi:.3f} s against 64 x the fastest per-song time {los / 8 * 64:.3f} s: "
                f"{'faster in every round' if ok else 'NOT faster by more than the spread'}")
        banks[n].trace_kernels = True
        banks[n].render_batch([F] * 8)
        banks[n].trace_kernels = False
        say(f"bank: N = {n}: kernels of one batch of 8 buffers: {', '.join(banks[n].last_kernels)}; overflows {banks[n].overflows()}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--only", choices=["mix", "bank"])
    ap.add_argument("--songs", default="64,1024")
    ap.add_argument("--song", default=os.path.join(ROOT, "tests", "golden", "example_song.txt"))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("song_bank_bench: no GPU; nothing is measured without one")
    import zang_amd
    ctx = zang_amd.default_context()
    say(f"device: {torch.cuda.get_device_name(0)}")
    ok = True
    if a.only != "bank":
        ok = bench_mix(ctx, a.rounds) and ok
    if a.only != "mix":
        ok = bench_bank(ctx, a.rounds, a.seconds, [int(x) for x in a.songs.split(",")], open(a.song).read()) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(LINES) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
