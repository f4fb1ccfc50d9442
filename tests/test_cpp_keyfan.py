"""CPU: the key fan-out stage's lane steps (zang_amd/csrc/keyfan_lane.hip.h, the text k_keyfan_schedule runs) and the stages' row
writer (span_stage.hip.h) compiled for the host with ASan and UBSan into a stand-alone program (tests/cpp/keyfan_lane_host.cpp) and
run over the case list with 66 players: the tables, counts, dropped rows and state words it prints after each of the six buffers
are the model's (tests/polyphony_reference.py).  No sanitizer enters Python."""
import os
import subprocess

import pytest

from tests import polyphony_cases as pc
from tests import polyphony_reference as pr
from tests.hostprog import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "keyfan_lane_host.cpp")
PLAYERS = 66


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("keyfan_lane"))


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def _input(case, outer, n, in_spans=pc.OUTER_SPANS):
    """outer: [buffer][player] -> [(s, e, mask, ...)]"""
    lines = [f"{case.n_keys} {pc.OUT_LEN} {case.max_spans} {n} {len(outer)} {in_spans}", " ".join(str(pr.bits(f)) for f in case.key_freqs())]
    for per_player in outer:
        for spans in per_player[:n]:
            row = [str(len(spans))]
            for s, e, m, *_ in spans:
                row += [str(s), str(e), str(m & 0xffffffff), str(m >> 32)]
            lines.append(" ".join(row))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_the_lane_equals_the_model_after_every_buffer(harness, case):
    rec = pc.run(case)
    out = _run(harness, _input(case, rec.outer, PLAYERS))
    assert out[-2] == "PASS", out[:2]
    V = PLAYERS * case.n_keys
    i = 0
    for b in range(pc.BUFFERS):
        ref, dropped = pr.table(pc.voices_of(rec.inner[b], case, PLAYERS), case.max_spans)
        assert out[i] == f"B {b} dropped {dropped}", (b, out[i])
        i += 1
        for v in range(V):
            head = [int(x) for x in out[i].split()[1:]]
            assert out[i].startswith("V ") and head == [int(ref["count"][v])] + rec.words[b][v], (b, v, out[i], rec.words[b][v])
            i += 1
            for k in range(head[0]):
                on = int(ref["note_on"][k, v])
                want = [int(ref["start"][k, v]), int(ref["end"][k, v]), pr.bits(ref["freq"][k, v]), on, int(ref["nic"][k, v]), on]
                assert out[i].startswith("R ") and [int(x) for x in out[i].split()[1:]] == want, (b, v, k, out[i], want)
                i += 1


def test_a_callers_table_the_outer_trigger_cannot_make(harness):
    """what include/zang_hip.h defines beyond the reference, read off Polyphony.paint and Trigger.next by hand: an EMPTY sub-span
    still draws the id and sets `down` but walks nothing (the impulse is lost, the carried note stays); a sub-span that ends before
    it starts or beyond the buffer ends the player's list"""
    case = pc.Case("by_hand", 2, 8, 0)
    f0, f1 = (pr.bits(f) for f in case.key_freqs())
    outer = [[[(0, 100, 0b01), (100, 100, 0b10), (100, 256, 0b10)]],          # key 0 down; an empty sub-span: key 0 up, key 1 down; the same mask
             [[(0, 10, 0b11), (20, 10, 0b00), (30, 40, 0b00)]],               # end < start: the list ends there
             [[(0, 10, 0b00), (10, 300, 0b11)]]]                              # end > out_len
    out = _run(harness, _input(case, outer, 1))
    assert out[-2] == "PASS"
    assert out[:-2] == [
        "B 0 dropped 0",
        f"V 2 3 0 1 1 {f0} 1", f"R 0 100 {f0} 1 1 1", f"R 100 256 {f0} 1 0 1",   # key 0: the note-off was lost, the note-on is carried
        "V 0 2 1 0 0 0 0",                                                       # key 1: down and an id drawn, no note
        "B 1 dropped 0",
        f"V 1 4 1 1 3 {f0} 1", f"R 0 10 {f0} 1 1 1",                             # key 0: bit 1 != down 0: a fresh note-on
        "V 0 2 1 0 0 0 0",                                                       # key 1: bit 1 == down 1, nothing carried
        "B 2 dropped 0",
        f"V 1 5 0 1 4 {f0} 0", f"R 0 10 {f0} 0 1 0",
        f"V 1 3 0 1 2 {f1} 0", f"R 0 10 {f1} 0 1 0",
    ]
