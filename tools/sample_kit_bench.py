"""GPU box: what a run-time format and a per-lane descriptor cost -- k_sampler_kit_spans (zh_sampler_paint_kit_spans) beside the
per-format k_sampler_spans (zh_sampler_paint_spans) on the same sample and the same table.
usage: sample_kit_bench.py [rounds]
Per voice count (4,096 and 131,072) x 1,024 frames, zero-first, one full-buffer sub-span per voice, HIP-event time per call (blocks of 4 calls), median of
`rounds` interleaved rounds (kit, plain, kit, plain, ...):
  uniform   every voice on ONE s16 mono sample of 1 s (kit entry 0): kit kernel against the per-format kernel, at the native rate (the
            plain path, Sampler.zig:105-114) and at per-voice rates of 0.5-1.5 x (the linear resampler, :116-130);
  mixed     the seven-entry layout of tests/sample_kit_cases.py (u8, s16 stereo, s24, s32 x 3 channels, an empty sample, one frame,
            s24 stereo) scaled to about 1 s per sample, voice v on entry v % 7, channel 0: the divergent case, kit kernel only."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = 1024
CALLS = 4            # per timed block: the queue stays full while the host builds the next call


def main(rounds):
    import numpy as np
    import torch
    import zang_amd
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf, as_f32
    from zang_amd.samplekit import SampleKit
    ctx = zang_amd.default_context()
    rng = np.random.default_rng(14)
    n = 44100
    spec = [(1, 44100, 1, n * 2), (1, 44100, 0, n), (2, 44100, 1, n * 4), (1, 22050, 2, n // 2 * 3 + 2), (3, 48000, 3, 48000 * 12), (1, 44100, 1, 0),
            (1, 44100, 1, 2), (2, 44100, 2, n * 6 + 5)]
    kit = SampleKit(ctx, [(c, r, f, rng.integers(0, 256, b, dtype=np.uint8)) for c, r, f, b in spec])
    span = zang.Span(0, F)

    def event_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record(); ctx.sync()
        return a.elapsed_time(b) * 1000.0 / CALLS

    for V in (4096, 131072):
        out = ctx.image(F, V, fill=0.0)
        m = mod.Sampler(V, ctx)
        outs = (abi.Buf * 1)(as_buf(out))
        ones, zeros, ends = np.ones(V), np.zeros((1, V)), np.full((1, V), F)
        for label, rate in (("native rate", np.full((1, V), 44100.0, np.float32)), ("0.5-1.5 x", rng.uniform(22050.0, 66150.0, (1, V)).astype(np.float32))):
            loop = np.ones((1, V), np.uint32)
            tk = m.kit_span_table(ones, zeros, ends, zeros, {"sample_rate": (rate, None), "loop": (None, loop)})
            tp = m.span_table(ones, zeros, ends, zeros, {"sample_rate": (rate, None), "loop": (None, loop)})
            ctb, sp = tp.device(ctx.device, ["sample_rate", "loop"])
            cp = abi.SamplerParams(as_f32(1.0), kit.sample(0), 0, 1, 0)
            kp = m.KitParams(kit, 1.0, 0, 0, True)
            f_kit = lambda: m.paint_kit_spans(span, [out], None, kp, tk, zero_first=True)
            f_plain = lambda: abi.check(ctx.lib.zh_sampler_paint_spans(m.handle, 0, F, outs, None, C.byref(cp), sp, C.byref(ctb), abi.PAINT_ZERO_FIRST), "plain")
            f_kit(); f_plain(); ctx.sync()
            a, b = [], []
            for _ in range(rounds):
                a.append(event_us(f_kit)); b.append(event_us(f_plain))
            ka, pb = statistics.median(a), statistics.median(b)
            print("uniform s16 mono, %-11s V=%6d  kit %8.1f us  per-format %8.1f us  (%.2f x)" % (label, V, ka, pb, ka / pb), flush=True)
        smp = (np.arange(V) % 7 + 1).astype(np.uint32)[None, :]
        for label, rate in (("native rate", np.array([spec[s][1] for s in smp[0]], np.float32)[None, :]), ("0.5-1.5 x", rng.uniform(22050.0, 66150.0, (1, V)).astype(np.float32))):
            tk = m.kit_span_table(ones, zeros, ends, zeros, {"sample_rate": (rate, None), "loop": (None, np.ones((1, V), np.uint32)), "sample": (None, smp)})
            kp = m.KitParams(kit, 1.0, 0, 0, True)
            f_kit = lambda: m.paint_kit_spans(span, [out], None, kp, tk, zero_first=True)
            f_kit(); ctx.sync()
            print("mixed seven-entry kit, %-11s V=%6d  kit %8.1f us" % (label, V, statistics.median(event_us(f_kit) for _ in range(rounds))), flush=True)
        m.close()
        del out
        torch.cuda.synchronize()
    kit.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
