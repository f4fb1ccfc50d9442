"""CPU: the merge stage's lane walk (zang_amd/csrc/merge_lane.hip.h, the text k_span_merge runs, its row stores included) compiled
for the host with ASan and UBSan into a stand-alone program (tests/cpp/merge_lane_host.cpp) and run over the case list for 66
players: the rows, counts and dropped rows it prints are the model's (tests/two_reference.py) -- the hand-written cases, random
tables of up to 34 rows per source at out_len 256, max_spans values that overflow, both field shapes.  The two-source voice's
state layout runs in the layout harness (tests/cpp/dual_state_host.cpp).  No sanitizer enters Python."""
import os
import subprocess

import pytest

from tests import two_cases as tc
from tests import two_reference as tr
from tests.hostprog import build_sanitized, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLER_START = 0xdead0001


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(os.path.join(ROOT, "tests", "cpp", "merge_lane_host.cpp"), tmp_path_factory.mktemp("merge_lane"))


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def _input(pa, pb, shape, out_len, max_spans, rows, spans_a, spans_b):
    lines = [f"{len(pa)} {out_len} {max_spans} {rows} {len(shape.kinds_a)} {shape.on_a} {spans_a} {len(shape.kinds_b)} {shape.on_b} {spans_b} "
             f"{FILLER_START} {out_len}"]
    for a, b in zip(pa, pb):
        for src in (a, b):
            row = [str(len(src))]
            for s, e, nic, w in src:
                row += [str(s), str(e), str(nic)] + [str(x) for x in w]
            lines.append(" ".join(row))
    return "\n".join(lines) + "\n"


def check(out, ref, dropped, n):
    """the harness's output against the model's table"""
    assert out[0] == f"dropped {dropped}" and out[-2] == "PASS", (out[0], dropped)
    i = 1
    for p in range(n):
        assert out[i] == f"P {int(ref['count'][p])}", (p, out[i], int(ref["count"][p]))
        i += 1
        for k in range(int(ref["count"][p])):
            want = [int(ref["start"][k, p]), int(ref["end"][k, p]), int(ref["nic"][k, p])] + [int(x) for x in ref["words"][:, k, p]]
            assert out[i].startswith("R ") and [int(x) for x in out[i].split()[1:]] == want, (p, k, out[i], want)
            i += 1
    assert i == len(out) - 2


@pytest.mark.parametrize("max_spans", (tc.MAX_SPANS,) + tc.OVERFLOW_MAX_SPANS)
@pytest.mark.parametrize("shape", [tc.EXAMPLE, tc.WIDE], ids=["example", "wide"])
def test_the_lane_equals_the_model(harness, shape, max_spans):
    pa, pb = tc.players(tc.PLAYERS, shape)
    n_out = len(shape.kinds_a) + len(shape.kinds_b) + 3
    ref, dropped = tr.merge_table(pa, shape.on_a, pb, shape.on_b, tc.OUT_LEN, max_spans, n_out)
    assert (dropped > 0) == (max_spans < tc.MAX_SPANS)
    check(_run(harness, _input(pa, pb, shape, tc.OUT_LEN, max_spans, tc.MAX_SPANS, tc.SOURCE_SPANS, tc.SOURCE_SPANS)), ref, dropped, tc.PLAYERS)


@pytest.mark.parametrize("case", tc.HAND, ids=tc.HAND_IDS)
def test_the_lane_makes_the_hand_written_rows(harness, case):
    """one player, straight against the table written by hand"""
    out = _run(harness, _input([case.a], [case.b], tc.EXAMPLE, tc.OUT_LEN, 4, 4, 3, 3))
    assert out[0] == "dropped 0" and out[1] == f"P {len(case.expect)}" and out[-2] == "PASS"
    for k, (s, e, nic, w) in enumerate(case.expect):
        assert [int(x) for x in out[2 + k].split()[1:]] == [s, e, nic] + list(w), (k, out[2 + k])


def test_a_count_above_the_sources_rows_is_clamped(harness):
    """count = 5 in a table of 2 rows (in->max_spans = 2): the walk stops after the second row; ASan would see a third read"""
    a = [(0, 10, 1, (tc.F1, 1)), (10, 20, 0, (tc.F2, 1))]
    b = [(0, 256, 0, (tc.C1, 0))]
    lines = _input([a], [b], tc.EXAMPLE, tc.OUT_LEN, 4, 4, 2, 2).split("\n")
    assert lines[1].startswith("2 ")
    lines[1] = "5" + lines[1][1:]
    out = _run(harness, "\n".join(lines))
    assert out[:4] == ["dropped 0", "P 2", f"R 0 10 1 {tc.F1} 1 {tc.C1} 0 1 1 0", f"R 10 20 0 {tc.F2} 1 {tc.C1} 0 1 0 0"]


def test_the_voices_state_layout_under_the_sanitizers(tmp_path):
    run_sanitized(os.path.join(ROOT, "tests", "cpp", "dual_state_host.cpp"), tmp_path)
