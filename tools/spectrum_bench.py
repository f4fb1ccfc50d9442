#!/usr/bin/env python3
"""GPU box: zh_spectrum_plot (k_spectrum, csrc/spectrum.hip) per 1,024-frame buffer at 4,096 and 131,072 voices, in the four forms
the dispatch rows select (tile of 16 or 8 voices; two butterfly stages per pass or one), against two yardsticks:
  floor   the bytes a plot must move, 4 KiB read + 2 KiB written per voice, at the 6.0 TB/s the library's own read-and-write
          stream kernels reach
  torch   torch.fft.rfft(image, dim=0).real.abs().mul(1 / 1024).sqrt() on the same image: another algorithm, not bit-comparable,
          a yardstick for time only
HIP events around K back-to-back calls on one stream, every variant warmed up, the variants alternating in every round; medians
and ranges.  The images rotate through a ring larger than the caches.  The forms' bits are compared before anything is timed.
usage: tools/spectrum_bench.py [rounds]             -> a table on stdout
       tools/spectrum_bench.py --profile VOICES     -> a few plots in the default form and nothing else (for rocprofv3)"""
import os
import statistics
import sys

os.environ["ZH_ENV_LIVE"] = "1"                         # the dispatch rows are re-read at every call: one process times every form
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import zang_amd
from zang_amd import abi
from zang_amd.runtime import as_buf

PROFILE = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--profile" else 0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and not PROFILE else 9
F, BINS, K = 1024, 512, 20
FLOOR_RATE = 6.0e12
FORMS = [(16, 2), (8, 2), (16, 1), (8, 1)]
torch.cuda.set_stream(torch.cuda.Stream())
ctx = zang_amd.Context(0)


def plot(img, out):
    abi.check(ctx.lib.zh_spectrum_plot(ctx.handle, 0, as_buf(img), as_buf(out)), "zh_spectrum_plot")


def set_form(form):
    os.environ["ZH_FORMS"] = "spectrum_tile=%d,spectrum_stages=%d" % form


def timed(fn, imgs, outs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(K):
        fn(imgs[i % len(imgs)], outs[i % len(outs)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / K


def torch_route(img, out):
    out.copy_(torch.fft.rfft(img, dim=0)[:BINS].real.abs().mul(1.0 / 1024.0).sqrt())


if PROFILE:
    img, out = torch.rand((F, PROFILE), device=ctx.device) * 2 - 1, ctx.image(BINS, PROFILE, fill=0.0)
    for _ in range(3):
        plot(img, out)
    ctx.sync()
    print("3 zh_spectrum_plot of %d voices x %d frames (k_spectrum): expect %d bytes read and %d written per plot" % (PROFILE, F, PROFILE * F * 4, PROFILE * BINS * 4))
    sys.exit(0)

print("# %d frames per plot, %d plots per timed window (HIP events), %d alternating rounds, one MI355X; us per plot: median (min - max)" % (F, K, ROUNDS))
print("%-8s %-44s %28s %8s %10s" % ("voices", "form", "us/plot", "x floor", "TB/s"))
for V in (4096, 131072):
    nimg = max(2, min(16, (512 << 20) // (F * V * 4)))  # a ring of 512 MiB: an image is not still in a cache at its next plot
    imgs = [torch.rand((F, V), device=ctx.device) * 2 - 1 for _ in range(nimg)]
    outs = [ctx.image(BINS, V, fill=0.0) for _ in range(nimg)]
    want = None
    for form in FORMS:                                   # same bits in every form, and near torch's FFT
        set_form(form)
        plot(imgs[0], outs[0]); ctx.sync()
        got = outs[0].clone()
        assert want is None or torch.equal(got.view(torch.int32), want.view(torch.int32)), form
        want = got
    torch_route(imgs[0], outs[1]); ctx.sync()
    assert float((outs[1] - want).abs().max()) < 2e-2, "the two routes differ"
    cases = [("k_spectrum tile %2d, %d stage%s per pass" % (f[0], f[1], "s" if f[1] > 1 else ""), f) for f in FORMS] + [("torch.fft.rfft + real/abs/mul/sqrt", None)]

    def run(form):
        if form is None:
            return timed(torch_route, imgs, outs)
        set_form(form)
        return timed(plot, imgs, outs)
    for _, f in cases:
        run(f)
    times = {name: [] for name, _ in cases}
    for r in range(ROUNDS):
        for name, f in (cases if r % 2 == 0 else cases[::-1]):
            times[name].append(run(f))
    floor = V * (F + BINS) * 4 / FLOOR_RATE * 1e6
    print("%-8d %-44s %28.1f" % (V, "floor: 6 KiB per voice at 6.0 TB/s", floor))
    for name, _ in cases:
        med = statistics.median(times[name])
        print("%-8d %-44s %10.1f (%6.1f - %6.1f) %8.2f %10.2f" % (V, name, med, min(times[name]), max(times[name]), med / floor,
                                                               V * (F + BINS) * 4 / (med * 1e-6) / 1e12))
    del imgs, outs
os.environ.pop("ZH_FORMS", None)
