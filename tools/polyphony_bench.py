#!/usr/bin/env python3
"""The key-per-voice polyphony player on one GPU (lines for profiles/rNN/NOTES.md): N players x 41 keys x 1,024 frames per paint,
every player holding a chord of three keys, its Decimator in mode player % 7 (0 = bypass).  HIP events around runs of calls, the
routes alternating in one process after a warm-up:

  paint        one PolyphonyPlayer.paint: the live bank's schedule (with its host side: no new events), zh_keyfan_schedule,
               zh_nice_paint_spans over all N x 41 voices, zh_decimator_paint_groups
  fan-out      zh_keyfan_schedule alone
  voices       zh_nice_paint_spans alone
  decimated    zh_decimator_paint_groups alone, zero-first, on the image the voices painted
  group mix    zh_mixdown_groups, zero-first, on the same image: the yardstick -- it reads the same bytes and was there before
  decimator    zh_decimator_paint of N voices on an [frames][N] image, zero-first: what a composition runs behind the group mix (and a
               transposing copy between the two, which is not timed)

    python tools/polyphony_bench.py [--players 64,3197] [--rounds 7] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, KEYS, SR = 1024, 41, 48000.0
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


def bench(ctx, rounds, N):
    import numpy as np
    import torch
    from zang_amd import modules as mod, polyphony, zang
    V = N * KEYS
    freqs = (220.0 * 2.0 ** (np.arange(KEYS) / 12.0)).astype(np.float32)
    player = polyphony.PolyphonyPlayer(ctx, N, freqs)
    for p in range(N):
        for _ in range(p % 7):
            player.space(p)
        for k in (p % KEYS, (p + 4) % KEYS, (p + 7) % KEYS):           # the chord, all at frame 0
            player.key(p, k, True, 0)
    audio = player.paint(F)
    ctx.sync()
    assert player.overflows() == 0 and float(audio.abs().max()) > 0.1
    sp, image = zang.Span(0, F), player._image[:F]
    rows = torch.empty((N, F), dtype=torch.float32, device=ctx.device)
    bus, out = ctx.image(F, N), ctx.image(F, N)
    bus.uniform_(-1.0, 1.0)
    dec = mod.Decimator(N, ctx)
    rate = torch.tensor([polyphony.DEC_RATES[p % 7] or 2.0 * SR for p in range(N)], dtype=torch.float32, device=ctx.device)   # (mode 0: add and reset)
    dparams = dec.Params(SR, bus, rate)
    routes = {
        "paint (four calls)": lambda: player.paint(F),
        "fan-out (zh_keyfan_schedule)": lambda: player.stage.schedule(F, player.max_spans, player._outer),
        "voices (zh_nice_paint_spans)": lambda: player.voices.paint_spans(sp, [image], None, SR, player._table, zero_first=True),
        "decimated (zh_decimator_paint_groups)": lambda: player.dec.paint_groups(sp, player._audio, image, KEYS, SR, player._modes, zero_first=True),
        "group mix (zh_mixdown_groups)": lambda: zang.mixdownGroups(sp, rows, image, KEYS, zero_first=True, ctx=ctx),
        "decimator (zh_decimator_paint, N voices)": lambda: dec.paint(sp, [out], [], False, dparams, zero_first=True),
    }
    reps = 20 if V <= 16384 else 5
    kernels = {}
    for name, fn in routes.items():                                   # warm-up of everything timed below
        timed(torch, fn, reps)
        kernels[name] = ", ".join(ctx.last_form())
    t = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            t[name].append(timed(torch, fn, reps))
    say(f"polyphony: {N} players x {KEYS} keys = {V} voices x {F} frames, a chord of three keys a player, Decimator modes player % 7, "
        f"{rounds} alternating rounds of {reps} calls")
    med = {}
    for name in routes:
        med[name] = statistics.median(t[name])
        say(f"polyphony:   {name:42s} {med[name]:9.1f} us (min {min(t[name]):.1f}, max {max(t[name]):.1f})  [{kernels[name]}]")
    d, g, c = med["decimated (zh_decimator_paint_groups)"], med["group mix (zh_mixdown_groups)"], med["decimator (zh_decimator_paint, N voices)"]
    say(f"polyphony:   decimated / group mix = {d / g:.2f}; group mix + decimator = {g + c:.1f} us (no transposing copy timed): decimated is "
        f"{'below' if d < g + c else 'NOT below'} it; the image read: {4 * V * F / d / 1e6:.2f} TB/s decimated, {4 * V * F / g / 1e6:.2f} TB/s group mix")
    player.close(); dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--players", default="64,3197")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("polyphony_bench: no GPU; nothing is measured without one")
    import zang_amd
    ctx = zang_amd.default_context()
    say(f"device: {torch.cuda.get_device_name(0)}")
    for N in [int(x) for x in a.players.split(",")]:
        bench(ctx, a.rounds, N)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
