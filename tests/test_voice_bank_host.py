"""CPU: the voice bank's per-lane scheduling steps (zang_amd/csrc/sched_lane.hip.h -- the text k_voice_bank_schedule runs)
compiled for the host with AddressSanitizer + UBSan (tests/cpp/sched_lane_host.cpp): the reference's eight unit tests fed as
impulses, and seeded random songs against zh_poly_voice_schedule, buffer by buffer.  No tolerance: integers and copied words."""
import os
import subprocess

import numpy as np
import pytest

from tests import voice_bank_cases as vb
from tests.hostprog import build_sanitized

ROOT = vb.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "sched_lane_host.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("sched_lane"))


def _run(exe, args, text=None):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("case", vb.GOLDEN["trigger"], ids=lambda c: c["name"])
def test_trigger_reference_cases_through_the_lane_functions(harness, case):
    lines = [str(len(case["steps"]))]
    for step in case["steps"]:
        lines.append(str(len(step["impulses"])))
        for (frame, note_id, event_id), p in zip(step["impulses"], step["params"]):
            lines.append(f"{frame} {note_id} {event_id} {vb.f32bits(p)}")
    out = _run(harness, ["trigger"], "\n".join(lines) + "\n").split("\n")
    got, cur = [], None
    for ln in out:
        if ln.startswith("step"):
            cur = []
            got.append(cur)
        elif ln.strip():
            cur.append(tuple(int(x) for x in ln.split()))
    assert got == [[(s, e, vb.f32bits(p), int(ch)) for s, e, p, ch in step["expected"]] for step in case["steps"]]


@pytest.mark.parametrize("case", vb.GOLDEN["polyphony_dispatcher"], ids=lambda c: c["name"])
def test_dispatcher_reference_cases_through_the_lane_functions(harness, case):
    lines = [str(len(case["impulses"]))] + [f"{f} {nid} {eid} {1 if on else 0}" for (f, nid, eid), on in zip(case["impulses"], case["note_on"])]
    out = _run(harness, ["dispatch", str(case["polyphony"])], "\n".join(lines) + "\n")
    got = [[int(x) for x in ln.split(":")[1].split()] for ln in out.strip().split("\n")]
    assert got == case["expected_note_ids"]


def _song_through_harness(exe, tmp, P, rec, t, ids, frames, rows, sr=vb.SR):
    W = rec.dtype.itemsize // 4
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([P, W, vb.ON_OFFSET, len(t), np.float32(sr).view(np.uint32), rows, len(frames), 0], np.uint32).tobytes())
        f.write(np.asarray(frames, np.uint32).tobytes() + t.tobytes() + ids.tobytes() + rec.tobytes())
    _run(exe, ["song", fin, fout])
    raw = open(fout, "rb").read()
    cells, pos, out = rows * P, 0, []
    for _ in frames:
        d = {}
        for name, n, dt in (("count", P, np.uint32), ("start", cells, np.uint32), ("end", cells, np.uint32), ("words", cells * W, np.uint32),
                            ("note_on", cells, np.uint8), ("note_id_changed", cells, np.uint8)):
            a = np.frombuffer(raw, dt, n, pos)
            pos += a.nbytes
            d[name] = a.reshape((W, rows, P) if name == "words" else (rows, P) if name != "count" else (P,))
        out.append(d)
    dropped = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
    assert pos + 8 == len(raw)
    return out, dropped


@pytest.mark.parametrize("polyphony", [1, 3, 8])
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_random_songs_equal_the_host_scheduler_buffer_by_buffer(harness, tmp_path, polyphony, dense):
    """72 buffers: 1,024 frames, odd lengths (a partial last buffer like write_wav's, 1 frame, 0 frames) in between."""
    frames = [1024] * 72
    for i, n in ((5, 1), (9, 777), (20, 0), (33, 1023), (50, 333), (71, 417)):
        frames[i] = n
    n_inst = 16 if dense else 1                              # instrument 15 of the corpus is a dense one
    offsets, rec, t, ids = vb.corpus(n_inst, len(frames), seed=vb.SEED + polyphony)
    a, b = int(offsets[n_inst - 1]), int(offsets[n_inst])
    rec, t, ids = rec[a:b].copy(), t[a:b].copy(), ids[a:b].copy()
    got, dropped = _song_through_harness(harness, str(tmp_path), polyphony, rec, t, ids, frames, 34)
    host = vb.HostBank(polyphony, np.array([0, len(t)], np.uint64), rec, t, ids)
    spans = 0
    for bi, n in enumerate(frames):
        ref = host.schedule([n])
        vb.assert_tables_equal(got[bi], ref, f"buffer {bi}")
        spans += int(ref["count"].sum())
    host.close()
    assert dropped == 0 and spans > len(frames)


def test_overflow_clamps_counts_and_keeps_the_trigger_state(harness, tmp_path):
    """rows = 2: every list stops at 2, the dropped sub-spans are counted, and what the first two rows hold still equals the host's
    in every later buffer (the Trigger state advanced as if every sub-span had been emitted)."""
    frames = [1024] * 16
    offsets, rec, t, ids = vb.corpus(16, len(frames))
    a, b = int(offsets[15]), int(offsets[16])
    rec, t, ids = rec[a:b].copy(), t[a:b].copy(), ids[a:b].copy()
    got, dropped = _song_through_harness(harness, str(tmp_path), 3, rec, t, ids, frames, 2)
    host = vb.HostBank(3, np.array([0, len(t)], np.uint64), rec, t, ids)
    beyond = 0
    for bi, n in enumerate(frames):
        ref = host.schedule([n])
        beyond += int(np.maximum(ref["count"].astype(np.int64) - 2, 0).sum())
        ref["count"] = np.minimum(ref["count"], 2)
        vb.assert_tables_equal(got[bi], ref, f"buffer {bi}")
    host.close()
    assert beyond > 0 and dropped == beyond
