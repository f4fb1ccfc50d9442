"""GPU box: kernel time of the builtin modules' span paints (k_<module>_spans, zh_<module>_paint_spans) against the plain paints.
usage:
  module_spans_bench.py run [reps] [manifest.json]   -- the launches; writes which kernels every timed block launched, in order
  module_spans_bench.py report manifest.json kernel_trace.csv   -- median kernel time per block from a rocprofv3 kernel trace
Run the first under `rocprofv3 --kernel-trace --stats -- python tools/module_spans_bench.py run`: the trace's dispatches, in
order, are those of the manifest's blocks (nothing else launches a kernel while they run).  Per module, 4,096 and 131,072 voices,
1,024-frame buffers, zero-first:
  (a) zh_<module>_paint, as dispatched (whatever form the library picks);
  (b) the spans form, one full-buffer sub-span per voice;
  (c) the spans form on the table of a polyphonic schedule (zh_poly_voice, 3 notes per voice over 4 buffers, its third buffer);
  (d) the spans form on random 0-3 sub-spans per voice (adjacent, gapped, empty, at the buffer's edges).
Every span field has an array in (c) and (d); (b) uses the plain paint's params.  The run also prints HIP-event times per call."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, SR = 1024, 48000.0
MODULES = ["sineosc", "pulseosc", "trisawosc", "noise", "envelope", "gate", "filter", "sampler", "decimator", "distortion"]


def run(reps, manifest_path):
    import ctypes as C
    import numpy as np
    import torch
    import zang_amd
    from zang_amd import abi, zang
    from tests.module_spans_cases import CASES, K, _arrays, _defaults, _tables
    ctx = zang_amd.default_context()
    blocks = []

    def timed(label, fn, n):
        fn(); ctx.sync()
        blocks.append({"label": label + " warm", "calls": 1, "kernels": ctx.last_form()})
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record(); ctx.sync()
        blocks.append({"label": label, "calls": n, "kernels": ctx.last_form()})
        return a.elapsed_time(b) * 1000.0 / n

    def poly_table(m, V, rng):
        """the third buffer of a zh_poly_voice schedule of 3 notes per voice over 4 buffers (freq and note_on per sub-span)"""
        n_ev = 3 * V
        t = np.sort(rng.uniform(0, 4 * F / SR, n_ev)).astype(np.float32)
        rec = np.zeros(n_ev, np.dtype({"names": ["freq", "note_on"], "formats": ["<f4", "u1"], "offsets": [0, 4], "itemsize": 8}))
        rec["freq"] = rng.uniform(100, 2000, n_ev); rec["note_on"] = rng.random(n_ev) < 0.7
        ids = np.arange(1, n_ev + 1, dtype=np.uint64)
        h = C.c_void_p()
        abi.check(m.lib.zh_poly_voice_create(V, 8, 4, n_ev, rec.ctypes.data, t.ctypes.data, ids.ctypes.data, C.byref(h)), "zh_poly_voice_create")
        cap = 34
        for _ in range(3):
            count = np.zeros(V, np.uint32); start = np.zeros((cap, V), np.uint32); end = np.zeros((cap, V), np.uint32)
            prm = np.zeros((cap, V), rec.dtype); nic = np.zeros((cap, V), np.uint8)
            fr = np.array([F], np.uint32)
            abi.check(m.lib.zh_poly_voice_schedule(h, SR, fr.ctypes.data, 1, cap, count.ctypes.data, start.ctypes.data, end.ctypes.data,
                                                   prm.ctypes.data, nic.ctypes.data), "zh_poly_voice_schedule")
        m.lib.zh_poly_voice_destroy(h)
        Kb = max(int(count.max()), 1)
        return count, start[:Kb], end[:Kb], nic[:Kb], float(count.mean())

    for name in MODULES:
        for V in (4096, 131072):
            case = CASES[name]()
            rng = np.random.default_rng(V)
            case.dflt = _defaults(case, rng, V)
            m = case.make(ctx, V)
            extra = {"input": ctx.image(F, V, fill=0.25)} if case.inputs else {}
            params = case.params(m, case.dflt, extra)
            out = ctx.image(F, V, fill=0.0)
            sp = zang.Span(0, F)
            full = m.span_table(np.ones(V), np.zeros((1, V)), np.full((1, V), F), np.zeros((1, V)))
            pc, ps, pe, pn, per_voice = poly_table(m, V, rng)
            poly = m.span_table(pc, ps, pe, pn, {n: g(rng, ps.shape) for n, g in case.fields})
            rc, rs, re_, rn = _arrays(_tables(V, 1, V + 1)[0])
            rand = m.span_table(rc, rs, re_, rn, {n: g(rng, (K, V)) for n, g in case.fields})
            nic = torch.zeros(V, dtype=torch.uint8, device=out.device)
            for t in (full, poly, rand):                          # upload the tables before anything is timed
                t.device(out.device, [n for n, _ in m._span_fields])
            ctx.sync()
            lab = "%s V=%d" % (name, V)
            res = {"a": timed(lab + " (a)", lambda: m.paint(sp, [out], [], nic, params, zero_first=True), reps)}
            form = blocks[-1]["kernels"]
            res["b"] = timed(lab + " (b)", lambda: m.paint_spans(sp, [out], None, params, full, zero_first=True), reps)
            res["c"] = timed(lab + " (c)", lambda: m.paint_spans(sp, [out], None, params, poly, zero_first=True), reps)
            res["d"] = timed(lab + " (d)", lambda: m.paint_spans(sp, [out], None, params, rand, zero_first=True), reps)
            print("%-10s V=%6d  (a) %-28s %8.1f us  (b) %8.1f us (%.2f x)  (c) %8.1f us (%.2f x, %.2f sub-spans a voice)  (d) %8.1f us (%.2f x)"
                  % (name, V, ",".join(form), res["a"], res["b"], res["b"] / res["a"], res["c"], res["c"] / res["a"], per_voice,
                     res["d"], res["d"] / res["a"]), flush=True)
            m.close()
            del out, extra
            torch.cuda.synchronize()
    json.dump(blocks, open(manifest_path, "w"))


def report(manifest_path, trace_path):
    import csv
    import statistics
    import re
    blocks = json.load(open(manifest_path))
    names = {k for b in blocks for k in b["kernels"]}

    def base(kernel):                                     # "void k_filter_spans<true, FilterSpans<...> >(...)" -> "k_filter_spans"
        return re.sub(r"^(void\s+)?", "", kernel).split("<")[0].split("(")[0].strip()
    # (the torch fills and module set-up between blocks are not ours: only the kernels the blocks named are kept)
    rows = sorted((r for r in csv.DictReader(open(trace_path)) if base(r["Kernel_Name"]) in names), key=lambda r: int(r["Start_Timestamp"]))
    i = 0
    med = {}
    for b in blocks:
        per_call = len(b["kernels"])
        n = b["calls"] * per_call
        chunk = rows[i:i + n]
        i += n
        for r, k in zip(chunk, b["kernels"] * b["calls"]):
            assert base(r["Kernel_Name"]) == k, (b["label"], k, r["Kernel_Name"])
        if b["label"].endswith("warm"):
            continue
        calls = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in chunk[c * per_call:(c + 1) * per_call]) / 1000.0
                 for c in range(b["calls"])]
        med[b["label"]] = (statistics.median(calls), ",".join(b["kernels"]))
    assert i == len(rows), (i, len(rows))
    print("| module | voices | (a) plain paint: form | (a) us | (b) one sub-span | (c) poly schedule | (d) random 0-3 |")
    print("|---|---|---|---|---|---|---|")
    for name in MODULES:
        for V in (4096, 131072):
            lab = "%s V=%d" % (name, V)
            a, form = med[lab + " (a)"]
            cells = ["%.1f (%.2f x)" % (med[lab + " (%s)" % c][0], med[lab + " (%s)" % c][0] / a) for c in "bcd"]
            print("| %s | %d | %s | %.1f | %s |" % (name, V, form, a, " | ".join(cells)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20, sys.argv[3] if len(sys.argv) > 3 else "module_spans_manifest.json")
    else:
        report(sys.argv[2], sys.argv[3])
