"""GPU box: kernel time of a generated module's spans form (zs_paint_spans_<name>) against its lane form over the whole buffer.
usage: script_spans_bench.py [reps]  -- prints one line per (module, voices, case); under `rocprofv3 --kernel-trace --stats`
the kernel table gives the same launches.  Cases: (a) zs_paint_<name> over [0, 1024) with the lane form forced
(ZH_FORMS=script_pc=0,script_ranges=0); (b) the spans form, one full-buffer sub-span per voice; (c) the spans form on the table
of a dense polyphonic schedule (zh_poly_voice, 44,100 Hz); (d) the spans form on random 0-3 sub-spans per voice.  Also: how many
paint calls one buffer of the polyphony-8 schedule costs on the old route (one module object per voice, one paint per sub-span)."""
import os, sys, time
os.environ["ZH_ENV_LIVE"] = "1"
os.environ["ZH_FORMS"] = "script_pc=0,script_ranges=0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zang_amd
from zang_amd import script, zang
from tests.test_gpu_script_spans import _random_lists, _demo_events

F, SR = 1024, 44100.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ctx = zang_amd.default_context()
CASES = [("Pluck", "script_modules.txt", {"sample_rate": SR, "freq": 440.0, "note_on": True}),
         ("FilteredSawtooth", "script_modules.txt", {"sample_rate": SR, "freq": 440.0, "note_on": True, "cutoff": 0.3}),
         ("DemoPlayer", "example_script.txt", {"sample_rate": SR, "freq": 440.0, "note_on": True})]


def timed(fn):
    fn(); ctx.sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); ctx.sync()
    return a.elapsed_time(b) * 1000.0 / reps


def poly_table(m, V, rng):
    events = _demo_events(rng, V * 3, 4 * F / SR)
    pv = script.PolyScriptVoice(m, V, ["freq", "note_on"], events)
    t = None
    for _ in range(3):                                   # the third buffer: notes carried over, new ones starting
        t = pv.schedule(F, SR)
    pv.close()
    return t


for name, fn, params in CASES:
    text = open(os.path.join(ROOT, "tests", "golden", fn)).read()
    prog = script.ScriptProgram(text, ctx, filename=fn, only=[name], spans=True)
    for V in (4096, 131072):
        rng = np.random.default_rng(V)
        m = prog.module(name, V)
        out = ctx.image(F, V, fill=0.0)
        sp = zang.Span(0, F)
        full = script.ScriptSpanTable(m.params, np.ones(V), np.zeros((1, V)), np.full((1, V), F), np.zeros((1, V)))
        dense = poly_table(m, V, rng)
        rand = script.ScriptSpanTable.from_lists(m.params, _random_lists(rng, V, F, m.params, vary=False))
        res = {"a": timed(lambda: m.paint(sp, [out], None, False, params, zero_first=True))}
        assert ctx.last_form() == ["zs_paint_" + name], ctx.last_form()
        res["b"] = timed(lambda: m.paint_spans(sp, [out], full, params, zero_first=True))
        res["c"] = timed(lambda: m.paint_spans(sp, [out], dense, params, zero_first=True))
        res["d"] = timed(lambda: m.paint_spans(sp, [out], rand, params, zero_first=True))
        print("%-17s V=%6d  (a) lane %8.1f us  (b) spans, one sub-span %8.1f us (%.2f x)  (c) poly schedule %8.1f us (%.2f x, %.2f sub-spans a voice)"
              "  (d) random 0-3 %8.1f us (%.2f x)" % (name, V, res["a"], res["b"], res["b"] / res["a"], res["c"], res["c"] / res["a"],
                                                   float(dense.count.mean()), res["d"], res["d"] / res["a"]), flush=True)
        m.close()
    prog.close()

# the old route for polyphony 8: one module object per voice, one zh_script_module_paint per sub-span
rng = np.random.default_rng(8)
prog = script.ScriptProgram(open(os.path.join(ROOT, "tests", "golden", "example_script.txt")).read(), ctx, only=["DemoPlayer"], spans=True)
m = prog.module("DemoPlayer", 8)
pv = script.PolyScriptVoice(m, 8, ["freq", "note_on"], _demo_events(rng, 40, 8 * F / SR))
calls = [int(pv.schedule(F, SR).count.sum()) for _ in range(8)]
print("polyphony 8, 8 buffers: the old route makes %s paint launches per buffer (%d in all); the spans form makes 1 per buffer" % (calls, sum(calls)))
pv.close(); prog.close()
