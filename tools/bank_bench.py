#!/usr/bin/env python3
"""One buffer of polyphonic NiceInstrument voices from "events known" to "image painted", two routes in one process, alternating:
  (a) host   per-instrument zh_poly_voice_schedule, the tables assembled [span][voice], SpanTable.from_arrays upload,
             zh_nice_paint_spans -- the route without a voice bank
  (b) device zh_voice_bank_schedule + the same paint, the tables never leave the device
Host clock around work that ends in a synchronise; HIP events around the scheduling kernel alone and the paint alone.
    python tools/bank_bench.py [--instruments 16384] [--polyphony 8] [--buffers 50] [--rounds 3] [--song]
--song: the 17 sub-voices of the example song's shape instead (three instruments of polyphony 3, 10 and 4, one bank each).
--live: the scheduling alone when the events are PUSHED per buffer (the impulses the corpus's NoteTrackers deliver), three routes:
  (a) host   zh_impulse_queue_* -> zh_polyphony_dispatcher_dispatch -> zh_trigger_* per instrument, assemble, upload (from Python: call-bound;
             (a') is zh_poly_voice_schedule on the same events, one compiled call per instrument: what a compiled composition cannot beat)
  (b) live   zh_voice_bank_schedule_live: host sort, staging copy and kernel
  (c) song   zh_voice_bank_schedule on the same events known in advance"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REC = np.dtype([("freq", "<f4"), ("on", "u1"), ("pad", "u1", 3)])
SR, F, CAP = 48000.0, 1024, 34


def corpus(n, buffers, gap, seed):
    """event times = running sums of exponential gaps per instrument, note ids 1..6, note_on with probability 0.6"""
    rng = np.random.default_rng(seed)
    per = int(buffers * F / SR / gap * 1.25) + 8
    t = np.cumsum(rng.exponential(gap, (n, per)), axis=1).astype(np.float32).reshape(-1)
    rec = np.zeros(n * per, REC)
    rec["freq"] = rng.uniform(50, 2000, n * per)
    rec["on"] = rng.random(n * per) < 0.6
    ids = rng.integers(1, 7, n * per).astype(np.uint64)
    return np.arange(n + 1, dtype=np.uint64) * per, rec, t, ids


class HostRoute:
    def __init__(self, lib, ctx, P, offsets, rec, t, ids, nice):
        from zang_amd import abi
        self.lib, self.ctx, self.P, self.n, self.nice = lib, ctx, P, len(offsets) - 1, nice
        self.handles = []
        for i in range(self.n):
            a, b = int(offsets[i]), int(offsets[i + 1])
            h = C.c_void_p()
            abi.check(lib.zh_poly_voice_create(P, 8, 4, b - a, rec[a:b].ctypes.data, t[a:b].ctypes.data, ids[a:b].ctypes.data, C.byref(h)), "create")
            self.handles.append(h)
        n = self.n
        self.count = np.zeros((n, P), np.uint32)
        self.start = np.zeros((n, CAP, P), np.uint32); self.end = np.zeros((n, CAP, P), np.uint32)
        self.rec = np.zeros((n, CAP, P), REC); self.nic = np.zeros((n, CAP, P), np.uint8)
        self.fr = np.array([F], np.uint32)
        self.args = [(h, self.count[i].ctypes.data, self.start[i].ctypes.data, self.end[i].ctypes.data, self.rec[i].ctypes.data, self.nic[i].ctypes.data)
                     for i, h in enumerate(self.handles)]

    def reset(self):
        for h in self.handles:
            self.lib.zh_poly_voice_reset(h)

    def buffer(self, image, span):
        from zang_amd.spans import SpanTable
        t0 = time.perf_counter()
        f, frp, sr = self.lib.zh_poly_voice_schedule, self.fr.ctypes.data, float(SR)
        for h, c, s, e, r, n in self.args:
            if f(h, sr, frp, 1, CAP, c, s, e, r, n):
                raise RuntimeError("zh_poly_voice_schedule")
        t1 = time.perf_counter()
        V = self.n * self.P
        count = self.count.reshape(V)
        K = max(int(count.max()), 1)
        tr = lambda a: np.ascontiguousarray(a[:, :K].transpose(1, 0, 2)).reshape(K, V)
        table = SpanTable.from_arrays(count, tr(self.start), tr(self.end), tr(self.rec["freq"]), tr(self.rec["on"]), tr(self.nic), self.ctx.device)
        t2 = time.perf_counter()
        self.nice.paint_spans(span, [image], None, SR, table, zero_first=True)
        self.ctx.sync()
        t3 = time.perf_counter()
        return t1 - t0, t2 - t1, t3 - t2

    def close(self):
        for h in self.handles:
            self.lib.zh_poly_voice_destroy(h)


def run(ctx, shapes, buffers, rounds, warmup, seed, out):
    import torch
    from zang_amd import bank as zbank, modules as mod, zang
    span = zang.Span(0, F)
    parts = []
    for k, (n, P) in enumerate(shapes):
        offsets, rec, t, ids = corpus(n, buffers + warmup, 0.004, seed + k)
        V = n * P
        nice_h, nice_d, nice_e = (mod.NiceInstrument(V, 0.25, ctx) for _ in range(3))    # (a), (b), and (b) under events: each its own history
        parts.append({"host": HostRoute(ctx.lib, ctx, P, offsets, rec, t, ids, nice_h), "bank": zbank.VoiceBank(ctx, P, rec, offsets, t, ids, 4, rows=CAP),
                      "nice_d": nice_d, "nice_e": nice_e, "img_h": ctx.image(F, V), "img_d": ctx.image(F, V), "events": len(t)})
    for p in parts:
        p["table"] = p["bank"].span_table(CAP, 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    stream = ctx._stream
    res = {"host": [], "device": [], "host_parts": [], "sched_kernel_us": [], "paint_us": []}
    for r in range(rounds):
        for p in parts:
            p["host"].reset(); p["bank"].reset()
        ctx.sync()
        for b in range(warmup + buffers):                       # route (a)
            t0 = time.perf_counter()
            hp = [p["host"].buffer(p["img_h"], span) for p in parts]
            dt = time.perf_counter() - t0
            if b >= warmup:
                res["host"].append(dt); res["host_parts"].append(np.sum(hp, axis=0))
        for b in range(warmup + buffers):                       # route (b)
            t0 = time.perf_counter()
            for p in parts:
                p["bank"].schedule([F], SR, CAP)
                p["nice_d"].paint_spans(span, [p["img_d"]], None, SR, p["table"], zero_first=True)
            ctx.sync()
            dt = time.perf_counter() - t0
            if b >= warmup:
                res["device"].append(dt)
        same = all(torch.equal(p["img_h"], p["img_d"]) for p in parts)      # both routes ended on the same buffer
        assert same, "the two routes painted different images"
        for p in parts:
            p["bank"].reset()
        for b in range(warmup + buffers):                       # route (b) again with events around each kernel
            s_us = p_us = 0.0
            for p in parts:
                ev[0].record(stream); p["bank"].schedule([F], SR, CAP); ev[1].record(stream)
                p["nice_e"].paint_spans(span, [p["img_d"]], None, SR, p["table"], zero_first=True); ev[2].record(stream)
                ctx.sync()
                s_us += ev[0].elapsed_time(ev[1]) * 1e3; p_us += ev[1].elapsed_time(ev[2]) * 1e3
            if b >= warmup:
                res["sched_kernel_us"].append(s_us); res["paint_us"].append(p_us)
        hs, ds = np.array(res["host"][-buffers:]), np.array(res["device"][-buffers:])
        print(f"round {r}: host {np.median(hs) * 1e3:9.3f} ms/buffer (min {hs.min() * 1e3:.3f})   device {np.median(ds) * 1e3:9.3f} ms/buffer (min {ds.min() * 1e3:.3f})",
              file=out, flush=True)
    hp = np.median(np.array(res["host_parts"]), axis=0) * 1e3
    h, d = np.median(res["host"]) * 1e3, np.median(res["device"]) * 1e3
    print(f"shapes {shapes}: {sum(n * P for n, P in shapes)} voices, {sum(p['events'] for p in parts)} events, {rounds} x {buffers} buffers per route, images equal", file=out)
    print(f"  (a) host route   median {h:9.3f} ms/buffer = schedule calls {hp[0]:.3f} + assemble/upload {hp[1]:.3f} + paint/sync {hp[2]:.3f}", file=out)
    print(f"  (b) device route median {d:9.3f} ms/buffer   ({h / d:.1f}x)", file=out)
    print(f"  HIP events: scheduling kernel median {np.median(res['sched_kernel_us']):.1f} us (min {np.min(res['sched_kernel_us']):.1f}), "
          f"paint median {np.median(res['paint_us']):.1f} us (min {np.min(res['paint_us']):.1f})", file=out, flush=True)
    for p in parts:
        assert p["bank"].overflows() == 0
        p["host"].close(); p["bank"].close()


def run_live(ctx, n, P, buffers, warmup, host_buffers, seed, out):
    """one buffer of pushed impulses for n instruments, three routes (module docstring); (b)'s tables are checked against (c)'s"""
    import torch
    from zang_amd import abi, bank as zbank
    from zang_amd.spans import SpanTable
    L = ctx.lib
    total = warmup + buffers
    offsets, rec, t, ids = corpus(n, total, 0.004, seed)
    V = n * P
    # what the NoteTrackers deliver, per buffer, in time order over all instruments (each instrument's own order kept)
    trackers, batches = [], [[] for _ in range(total)]
    for i in range(n):
        a, z = int(offsets[i]), int(offsets[i + 1])
        h = C.c_void_p()
        abi.check(L.zh_note_tracker_create(8, z - a, rec[a:z].ctypes.data, t[a:z].ctypes.data_as(C.POINTER(C.c_float)),
                                           ids[a:z].ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(h)), "create")
        trackers.append(h)
    iap = abi.Iap()
    for b in range(total):
        for i, h in enumerate(trackers):
            if L.zh_note_tracker_consume(h, float(SR), 0, F, C.byref(iap)):
                raise RuntimeError("zh_note_tracker_consume")
            k = int(iap.len)
            assert k < 32
            if k:
                imp = np.frombuffer(C.string_at(iap.impulses, k * 24), np.uint64).reshape(k, 3)
                batches[b].append((np.full(k, i, np.uint32), imp[:, 0].astype(np.uint32), imp[:, 1].copy(), np.frombuffer(C.string_at(iap.paramses, k * 8), REC)))
    for h in trackers:
        L.zh_note_tracker_destroy(h)
    for b in range(total):
        inst, frame, nid, recs = (np.concatenate(x) for x in zip(*batches[b]))
        order = np.argsort(frame, kind="stable")
        batches[b] = tuple(np.ascontiguousarray(x[order]) for x in (inst, frame, nid, recs))
    most = max(len(x[0]) for x in batches)
    live = zbank.LiveVoiceBank(ctx, n, P, REC, 4, most, rows=CAP)
    song = zbank.VoiceBank(ctx, P, rec, offsets, t, ids, 4, rows=CAP)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = ctx._stream
    res = {"b_call": [], "b_total": [], "b_dev_us": [], "c_total": [], "c_dev_us": []}
    for b in range(total):
        inst, frame, nid, recs = batches[b]
        c = abi.BankImpulses(len(inst), inst.ctypes.data, frame.ctypes.data, nid.ctypes.data, recs.ctypes.data)
        ctx.sync()
        t0 = time.perf_counter()
        ev[0].record(stream)
        abi.check(L.zh_voice_bank_schedule_live(live.handle, F, CAP, C.byref(c)), "zh_voice_bank_schedule_live")
        t1 = time.perf_counter()
        ev[1].record(stream)
        ctx.sync()
        t2 = time.perf_counter()
        dev_b = ev[0].elapsed_time(ev[1]) * 1e3
        t3 = time.perf_counter()
        ev[0].record(stream)
        song.schedule([F], SR, CAP)
        ev[1].record(stream)
        ctx.sync()
        t4 = time.perf_counter()
        if b >= warmup:
            res["b_call"].append(t1 - t0); res["b_total"].append(t2 - t0); res["b_dev_us"].append(dev_b)
            res["c_total"].append(t4 - t3); res["c_dev_us"].append(ev[0].elapsed_time(ev[1]) * 1e3)
    dl, ds = live.download(CAP), song.download(CAP)
    K = int(ds["count"].max())
    m = np.arange(K, dtype=np.uint32)[:, None] < ds["count"][None, :]
    assert np.array_equal(dl["count"], ds["count"]) and all(np.array_equal(dl[k][:K][m], ds[k][:K][m]) for k in ("start", "end", "note_on", "note_id_changed"))
    assert all(np.array_equal(dl["words"][w][:K][m], ds["words"][w][:K][m]) for w in range(2)) and live.overflows() == 0 and song.overflows() == 0
    # (a): the host classes from Python, per instrument; (a'): one compiled call per instrument on the same events
    queues, disps, trigs = [], [], []
    for i in range(n):
        q, d = C.c_void_p(), C.c_void_p()
        abi.check(L.zh_impulse_queue_create(8, C.byref(q)), "create"); abi.check(L.zh_polyphony_dispatcher_create(P, 8, 4, C.byref(d)), "create")
        ts = []
        for _ in range(P):
            h = C.c_void_p()
            abi.check(L.zh_trigger_create(8, C.byref(h)), "create")
            ts.append(h)
        queues.append(q); disps.append(d); trigs.append(ts)
    poly, ps = (abi.Iap * P)(), abi.PaintSpan()
    push, consume, dispatch, counter, nxt = L.zh_impulse_queue_push, L.zh_impulse_queue_consume, L.zh_polyphony_dispatcher_dispatch, L.zh_trigger_counter, L.zh_trigger_next
    a_parts = []
    for b in range(min(host_buffers + 1, total)):
        inst, frame, nid, recs = batches[b]
        count = np.zeros(V, np.uint32)
        start = np.zeros((CAP, V), np.uint32); end = np.zeros((CAP, V), np.uint32); freq = np.zeros((CAP, V), np.float32)
        on = np.zeros((CAP, V), np.uint8); nic = np.zeros((CAP, V), np.uint8)
        t0 = time.perf_counter()
        base = recs.ctypes.data
        for k in range(len(inst)):
            push(queues[inst[k]], int(frame[k]), int(nid[k]), base + 8 * k)
        for i in range(n):
            consume(queues[i], C.byref(iap))
            dispatch(disps[i], iap, poly)
            for s in range(P):
                v = i * P + s
                counter(trigs[i][s], 0, F, poly[s])
                r = 0
                while nxt(trigs[i][s], C.byref(ps)) == 1:
                    start[r, v] = ps.start; end[r, v] = ps.end; nic[r, v] = ps.note_id_changed
                    freq[r, v] = np.frombuffer(ps.params, np.float32, 1)[0]; on[r, v] = ps.params[4]
                    r += 1
                count[v] = r
        t1 = time.perf_counter()
        K = max(int(count.max()), 1)
        SpanTable.from_arrays(count, start[:K], end[:K], freq[:K], on[:K], nic[:K], ctx.device)
        ctx.sync()
        t2 = time.perf_counter()
        if b >= 1:
            a_parts.append((t1 - t0, t2 - t1))
    assert np.array_equal(count, song_count_at(ctx, n, P, offsets, rec, t, ids, min(host_buffers + 1, total)))
    for q in queues:
        L.zh_impulse_queue_destroy(q)
    for d in disps:
        L.zh_polyphony_dispatcher_destroy(d)
    for ts in trigs:
        for h in ts:
            L.zh_trigger_destroy(h)
    host = HostRoute(L, ctx, P, offsets, rec, t, ids, None)
    a2 = []
    for b in range(total):
        t0 = time.perf_counter()
        f, frp, sr = L.zh_poly_voice_schedule, host.fr.ctypes.data, float(SR)
        for h, c_, s_, e_, r_, n_ in host.args:
            if f(h, sr, frp, 1, CAP, c_, s_, e_, r_, n_):
                raise RuntimeError("zh_poly_voice_schedule")
        t1 = time.perf_counter()
        cnt = host.count.reshape(V)
        K = max(int(cnt.max()), 1)
        tr = lambda a: np.ascontiguousarray(a[:, :K].transpose(1, 0, 2)).reshape(K, V)
        SpanTable.from_arrays(cnt, tr(host.start), tr(host.end), tr(host.rec["freq"]), tr(host.rec["on"]), tr(host.nic), ctx.device)
        ctx.sync()
        t2 = time.perf_counter()
        if b >= warmup:
            a2.append((t1 - t0, t2 - t1))
    host.close()
    live.close(); song.close()
    ap, a2p = np.median(np.array(a_parts), axis=0) * 1e3, np.median(np.array(a2), axis=0) * 1e3
    med = lambda k, scale=1e3: float(np.median(res[k]) * scale)
    print(f"live: {n} instruments x polyphony {P} = {V} voices, one buffer of {F} frames, {int(np.mean([len(x[0]) for x in batches]))} impulses per buffer, "
          f"{buffers} buffers per route ({len(a_parts)} for (a)); (b) and (c) left identical tables", file=out)
    print(f"  (a)  host classes from Python  median {ap.sum():9.3f} ms/buffer = composition {ap[0]:.3f} + assemble/upload {ap[1]:.3f}", file=out)
    print(f"  (a') zh_poly_voice_schedule    median {a2p.sum():9.3f} ms/buffer = schedule calls {a2p[0]:.3f} + assemble/upload {a2p[1]:.3f}", file=out)
    print(f"  (b)  zh_voice_bank_schedule_live median {med('b_total'):7.3f} ms/buffer to the end of the kernel: the call (sort, staging, enqueue) {med('b_call'):.3f}, "
          f"HIP events around the call (they see the host sort too) {med('b_dev_us', 1):.1f} us (min {np.min(res['b_dev_us']):.1f})", file=out)
    print(f"  (c)  zh_voice_bank_schedule    median {med('c_total'):9.3f} ms/buffer, kernel by HIP events {med('c_dev_us', 1):.1f} us (min {np.min(res['c_dev_us']):.1f})", file=out, flush=True)


def song_count_at(ctx, n, P, offsets, rec, t, ids, n_buffers):
    """the song bank's counts after n_buffers buffers (what (a)'s last buffer must have produced)"""
    from zang_amd import bank as zbank
    b = zbank.VoiceBank(ctx, P, rec, offsets, t, ids, 4, rows=CAP)
    for _ in range(n_buffers):
        b.schedule([F], SR, CAP)
    c = b.download(CAP)["count"]
    b.close()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instruments", type=int, default=16384)
    ap.add_argument("--polyphony", type=int, default=8)
    ap.add_argument("--buffers", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--song", action="store_true")
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--host-buffers", type=int, default=3, help="--live: buffers of route (a), after one warm-up buffer")
    a = ap.parse_args()
    import zang_amd
    ctx = zang_amd.default_context()
    if a.live:
        run_live(ctx, a.instruments, a.polyphony, a.buffers, a.warmup, a.host_buffers, a.seed, sys.stdout)
        return
    shapes = [(1, 3), (1, 10), (1, 4)] if a.song else [(a.instruments, a.polyphony)]
    run(ctx, shapes, a.buffers, a.rounds, a.warmup, a.seed, sys.stdout)


if __name__ == "__main__":
    main()
