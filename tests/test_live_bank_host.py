"""CPU: the live voice bank's per-lane steps (zang_amd/csrc/sched_lane.hip.h -- the text k_voice_bank_schedule_live runs) compiled
for the host with AddressSanitizer + UBSan (tests/cpp/live_lane_host.cpp): the reference's eight unit tests fed as pushes, and the seeded
corpus of pushed impulses against the host classes composed per instrument (tests/live_bank_cases.py), buffer by buffer.  No tolerance:
integers and copied words."""
import os
import subprocess

import numpy as np
import pytest

from tests import live_bank_cases as lb
from tests import voice_bank_cases as vb
from tests.hostprog import build_sanitized

SRC = os.path.join(lb.ROOT, "tests", "cpp", "live_lane_host.cpp")
N_INST = 32                                      # instruments 15 and 31 of the corpus push 40 per buffer


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("live_lane"))


def _run(exe, args, text=None):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("case", lb.GOLDEN["trigger"], ids=lambda c: c["name"])
def test_trigger_reference_cases_as_pushes_through_the_live_lane_steps(harness, case):
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


@pytest.mark.parametrize("case", lb.GOLDEN["polyphony_dispatcher"], ids=lambda c: c["name"])
def test_dispatcher_reference_cases_as_pushes_through_the_live_lane_steps(harness, case):
    lines = [str(len(case["impulses"]))] + [f"{f} {nid} {eid} {1 if on else 0}" for (f, nid, eid), on in zip(case["impulses"], case["note_on"])]
    out = _run(harness, ["dispatch", str(case["polyphony"])], "\n".join(lines) + "\n")
    got = [[int(x) for x in ln.split(":")[1].split()] for ln in out.strip().split("\n")]
    assert got == case["expected_note_ids"]


def _through_harness(exe, tmp, n_inst, P, buffers, rows):
    """the corpus, each buffer's batch sorted by instrument (stable) as zh_voice_bank_schedule_live sorts it
    -> (tables per buffer, dropped sub-spans, final state)"""
    W = lb.W
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n_inst, P, W, lb.ON_OFFSET, rows, len(buffers), 0, 0], np.uint32).tobytes())
        for out_len, inst, frame, ids, rec in buffers:
            order = np.argsort(inst, kind="stable")
            offsets = np.concatenate([[0], np.cumsum(np.bincount(inst, minlength=n_inst))]).astype(np.uint32)
            f.write(np.array([out_len, len(inst)], np.uint32).tobytes() + offsets.tobytes() + frame[order].tobytes() + ids[order].tobytes() + rec[order].tobytes())
    _run(exe, ["bank", fin, fout])
    raw = open(fout, "rb").read()
    V = n_inst * P
    cells, pos, out = rows * V, 0, []

    def take(dt, n, shape=None):
        nonlocal pos
        a = np.frombuffer(raw, dt, n, pos)
        pos += a.nbytes
        return a.reshape(shape) if shape else a
    for _ in buffers:
        out.append({"count": take(np.uint32, V), "start": take(np.uint32, cells, (rows, V)), "end": take(np.uint32, cells, (rows, V)),
                    "words": take(np.uint32, cells * W, (W, rows, V)), "note_on": take(np.uint8, cells, (rows, V)),
                    "note_id_changed": take(np.uint8, cells, (rows, V))})
    dropped = int(take(np.uint64, 1)[0])
    state = {"next_event_id": take(np.uint64, n_inst), "flags": take(np.uint32, V), "slot_note": take(np.uint64, V), "slot_event": take(np.uint64, V),
             "trig_has": take(np.uint32, V), "trig_note": take(np.uint64, V), "carried": take(np.uint32, W * V, (W, V))}
    assert pos == len(raw)
    return out, dropped, state


class _Voice:
    """the harness's state of one voice in the shape lb.assert_state_equal reads"""

    def __init__(self, st, v):
        self.used, self.note_on = int(st["flags"][v]) & 1, (int(st["flags"][v]) >> 1) & 1
        self.note_id, self.event_id = int(st["slot_note"][v]), int(st["slot_event"][v])
        self.has_note, self.trigger_note_id = int(st["trig_has"][v]), int(st["trig_note"][v])
        self.carried = [int(x) for x in st["carried"][:, v]] + [0] * (16 - lb.W)


@pytest.mark.parametrize("polyphony", [1, 3, 8])
def test_corpus_equals_the_host_composition_buffer_by_buffer(harness, tmp_path, polyphony):
    """24 buffers of pushes (1,024 frames; single ones of 1, 0, 777 and 1,023) for 32 instruments: every table and the final state"""
    buffers = lb.corpus(N_INST)
    refs, host = lb.reference(N_INST, polyphony)
    lb.assert_coverage(host.stats, len(buffers))
    got, dropped, state = _through_harness(harness, str(tmp_path), N_INST, polyphony, buffers, lb.ROWS)
    for bi, ref in enumerate(refs):
        vb.assert_tables_equal(got[bi], ref, f"buffer {bi}")
    assert dropped == 0
    lb.assert_state_equal(state["next_event_id"], [_Voice(state, v) for v in range(N_INST * polyphony)], host, "final state")


def test_overflow_clamps_counts_and_keeps_the_trigger_state(harness, tmp_path):
    """rows = 2: every list stops at 2, the dropped sub-spans are counted, and what the first two rows hold still equals the reference's
    in every later buffer (Trigger state and carried records advanced as if every sub-span had been emitted)."""
    P = 3
    buffers = lb.corpus(N_INST)
    refs, _ = lb.reference(N_INST, P)
    got, dropped, _ = _through_harness(harness, str(tmp_path), N_INST, P, buffers, 2)
    beyond = 0
    for bi, ref in enumerate(refs):
        ref = dict(ref)
        beyond += int(np.maximum(ref["count"].astype(np.int64) - 2, 0).sum())
        ref["count"] = np.minimum(ref["count"], 2)
        vb.assert_tables_equal(got[bi], ref, f"buffer {bi}")
    assert beyond > 0 and dropped == beyond
