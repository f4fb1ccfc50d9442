"""Shared by tests/test_voice_bank_host.py (CPU) and tests/test_gpu_voice_bank.py: the seeded song corpus, the per-instrument
host reference (zh_poly_voice_schedule) assembled into bank-shaped tables, and the reference's eight unit tests as songs."""
import ctypes as C
import json
import os

import numpy as np

from zang_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "scheduler_tests.json")))
REC = np.dtype([("freq", "<f4"), ("on", "u1"), ("pad", "u1", 3)])       # examples/example_song.zig MyNoteParams {freq, note_on}
ON_OFFSET = 4
SEED = 20261016
SR = 48000.0


def corpus(n_instruments, n_buffers, seed=SEED, frames=1024, gap=0.004):
    """Per instrument: event times = running sum of exponential gaps (mean 4 ms; one instrument in 16 dense, mean 0.3 ms), note
    ids uniform in 1..6, note_on with probability 0.6, freq uniform.  -> offsets [n + 1] u64, records, t f32, note ids u64."""
    rng = np.random.default_rng(seed)
    ts, recs, ids, offsets = [], [], [], [0]
    for i in range(n_instruments):
        g = 0.0003 if i % 16 == 15 else gap
        n = int(n_buffers * frames / SR / g * 1.2) + 4
        ts.append(np.cumsum(rng.exponential(g, n)).astype(np.float32))
        r = np.zeros(n, REC)
        r["freq"] = rng.uniform(50, 2000, n)
        r["on"] = rng.random(n) < 0.6
        recs.append(r)
        ids.append(rng.integers(1, 7, n).astype(np.uint64))
        offsets.append(offsets[-1] + n)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return np.array(offsets, np.uint64), cat(recs, REC), cat(ts, np.float32), cat(ids, np.uint64)


class HostBank:
    """The parent's route: one zh_poly_voice per instrument; schedule() -> tables shaped like the bank's."""

    def __init__(self, polyphony, offsets, records, t, note_ids, note_on_offset=ON_OFFSET):
        self.lib = abi.load()
        self.P, self.n = polyphony, len(offsets) - 1
        self.rec_dtype = records.dtype
        self.W = records.dtype.itemsize // 4
        self.keep = (records, t, note_ids)
        self.handles = []
        for i in range(self.n):
            a, b = int(offsets[i]), int(offsets[i + 1])
            h = C.c_void_p()
            abi.check(self.lib.zh_poly_voice_create(polyphony, records.dtype.itemsize, note_on_offset, b - a,
                                                    records[a:b].ctypes.data if b > a else None, t[a:b].ctypes.data if b > a else None,
                                                    note_ids[a:b].ctypes.data if b > a else None, C.byref(h)), "zh_poly_voice_create")
            self.handles.append(h)
        self.on_word, self.on_shift = note_on_offset // 4, 8 * (note_on_offset % 4)

    def reset(self):
        for h in self.handles:
            abi.check(self.lib.zh_poly_voice_reset(h), "zh_poly_voice_reset")

    def schedule(self, frames, sample_rate=SR, cap=None):
        fr = np.atleast_1d(np.asarray(frames, np.uint32))
        P, V, W = self.P, self.n * self.P, self.W
        cap = cap or 34 * len(fr)
        out = {"count": np.zeros(V, np.uint32), "start": np.zeros((cap, V), np.uint32), "end": np.zeros((cap, V), np.uint32),
               "words": np.zeros((W, cap, V), np.uint32), "note_id_changed": np.zeros((cap, V), np.uint8)}
        count = np.zeros(P, np.uint32)
        start = np.zeros((cap, P), np.uint32); end = np.zeros((cap, P), np.uint32)
        rec = np.zeros((cap, P, W), np.uint32); nic = np.zeros((cap, P), np.uint8)
        for i, h in enumerate(self.handles):
            abi.check(self.lib.zh_poly_voice_schedule(h, float(sample_rate), fr.ctypes.data, len(fr), cap, count.ctypes.data, start.ctypes.data,
                                                      end.ctypes.data, rec.ctypes.data, nic.ctypes.data), "zh_poly_voice_schedule")
            s = slice(i * P, (i + 1) * P)
            out["count"][s] = count
            out["start"][:, s] = start; out["end"][:, s] = end; out["note_id_changed"][:, s] = nic
            out["words"][:, :, s] = rec.transpose(2, 0, 1)
        out["note_on"] = (((out["words"][self.on_word] >> self.on_shift) & 0xff) != 0).astype(np.uint8)
        return out

    def close(self):
        for h in self.handles:
            self.lib.zh_poly_voice_destroy(h)
        self.handles = []


def live(count, rows):
    """[rows][V] mask of the cells that hold a sub-span"""
    return np.arange(rows, dtype=np.uint32)[:, None] < count[None, :]


def assert_tables_equal(got, ref, what=""):
    """every array identical where a sub-span lives (rows at or above count are not defined)"""
    assert np.array_equal(got["count"], ref["count"]), (what, "count", np.flatnonzero(got["count"] != ref["count"])[:8])
    K = int(ref["count"].max()) if len(ref["count"]) else 0
    assert K <= got["start"].shape[0], (what, "rows", K)
    m = live(ref["count"], K)
    for name in ("start", "end", "note_on", "note_id_changed"):
        assert np.array_equal(got[name][:K][m], ref[name][:K][m]), (what, name)
    for w in range(ref["words"].shape[0]):
        assert np.array_equal(got["words"][w][:K][m], ref["words"][w][:K][m]), (what, "word", w)


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def trigger_case_song(case):
    """A Trigger case as a song for polyphony 1 at sample_rate 1024, 1,024-frame buffers: step b's impulse at `frame` is an
    event at t = b + frame / 1024 (exact in f32), every event a note-on.  -> (records, t, ids, expected per buffer)"""
    recs, ts, ids, expected = [], [], [], []
    for b, step in enumerate(case["steps"]):
        for (frame, note_id, _), p in zip(step["impulses"], step["params"]):
            recs.append((p, 1, (0, 0, 0))); ts.append(b + frame / 1024.0); ids.append(note_id)
        expected.append([(s, e, f32bits(p), int(ch)) for s, e, p, ch in step["expected"]])
    return np.array(recs, REC) if recs else np.zeros(0, REC), np.array(ts, np.float32), np.array(ids, np.uint64), expected


def dispatcher_case_song(case):
    """A PolyphonyDispatcher case as a one-buffer song: the note id also in the record's float word."""
    recs = [(float(i[1]), 1 if on else 0, (0, 0, 0)) for i, on in zip(case["impulses"], case["note_on"])]
    ts = [i[0] / 1024.0 for i in case["impulses"]]
    return np.array(recs, REC), np.array(ts, np.float32), np.array([i[1] for i in case["impulses"]], np.uint64)
