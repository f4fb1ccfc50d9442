"""CPU: the controlled phase-modulation voice's three-cursor walk (zang_amd/csrc/pmctl.hip.h pmctl_walk, the text both pmctl
kernels run) compiled for the host with ASan and UBSan into a stand-alone program (tests/cpp/pmctl_walk_host.cpp) and run over the
GPU tests' streams (tests/mouse_cases.py) and over rows written by hand: the events and segments it prints are the model's
(tests/mouse_reference.py segments).  The voice's state layout runs in its own harness (tests/cpp/pmctl_state_host.cpp).  No
sanitizer enters Python."""
import os
import subprocess

import pytest

from tests import mouse_cases as mc
from tests import mouse_reference as mr
from tests.hostprog import build_sanitized, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(os.path.join(ROOT, "tests", "cpp", "pmctl_walk_host.cpp"), tmp_path_factory.mktemp("pmctl_walk"))


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split("\n")
    assert out[-2] == "PASS"
    return out[:-2]


def _input(tables, span, K=None):
    V = len(tables[0]["count"])
    K = K or tables[0]["start"].shape[0]
    lines = [f"{V} {K} {span[0]} {span[1]} {mc.POISON}"]
    for tb in tables:
        for v in range(V):
            n = int(tb["count"][v])
            row = [str(n)]
            for k in range(min(n, K)):
                row += [str(int(tb["start"][k, v])), str(int(tb["end"][k, v])), str(int(tb["nic"][k, v]))]
            lines.append(" ".join(row))
    return "\n".join(lines) + "\n"


def _model(tables, span):
    lines = []
    for v in range(len(tables[0]["count"])):
        lines.append(f"V {v}")
        for ev in mr.segments(tables, v, *span):
            if ev[0] == "begin":
                lines.append(f"B {ev[1]} {ev[2]} {int(tables[ev[1]]['nic'][ev[2], v])}")
            elif ev[0] == "end":
                lines.append(f"E {ev[1]}")
            else:
                lines.append(f"S {ev[1]} {ev[2]} {ev[3]}")
    return lines


@pytest.mark.parametrize("F", [1, 7, 96])
def test_the_walk_equals_the_model_on_the_gpu_tests_streams(harness, F):
    for seed in range(8):                                              # every feature reaches every voice index
        tables = mc.streams(130, F, seed)
        got, want = _run(harness, _input(tables, mc.SPANS[F])), _model(tables, mc.SPANS[F])
        assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got + [""], want + [""])) if g != w)


def _hand(notes, ratio, mult):
    """one voice's three row lists [(start, end, nic)] -> tables"""
    tbs = [mc.table(1, "freq"), mc.table(1, "value"), mc.table(1, "value")]
    for tb, rows in zip(tbs, (notes, ratio, mult)):
        tb["count"][0] = len(rows)
        for k, (s, e, nic) in enumerate(rows):
            tb["start"][k, 0], tb["end"][k, 0], tb["nic"][k, 0] = s, e, nic
    return tbs


HAND = {
    "no_rows": (([], [], []), ["S 0 16 0"]),
    "one_stream": (([(4, 9, 1)], [], []), ["S 0 4 0", "B 0 0 1", "S 4 9 1", "E 0", "S 9 16 0"]),
    "unrelated_boundaries": (([(2, 10, 0)], [(0, 6, 1), (6, 16, 0)], [(5, 12, 1)]),
                             ["B 1 0 1", "S 0 2 2", "B 0 0 0", "S 2 5 3", "B 2 0 1", "S 5 6 7", "E 1", "B 1 1 0", "S 6 10 7", "E 0", "S 10 12 6",
                              "E 2", "S 12 16 2", "E 1"]),
    "all_three_end_on_one_frame": (([(0, 8, 1), (8, 16, 0)], [(0, 8, 0), (8, 16, 1)], [(3, 8, 1)]),
                                   ["B 0 0 1", "B 1 0 0", "S 0 3 3", "B 2 0 1", "S 3 8 7", "E 0", "B 0 1 0", "E 1", "B 1 1 1", "E 2", "S 8 16 3",
                                    "E 0", "E 1"]),
    "empty_rows": (([(4, 4, 1), (4, 6, 0)], [(16, 16, 1)], [(0, 0, 0)]),
                   ["B 2 0 0", "E 2", "S 0 4 0", "B 0 0 1", "E 0", "B 0 1 0", "S 4 6 1", "E 0", "S 6 16 0", "B 1 0 1", "E 1"]),
    "out_of_order_ends_that_stream_only": (([(0, 8, 1), (4, 12, 1), (12, 16, 1)], [(0, 16, 1)], [(2, 4, 0), (10, 16, 0)]),
                                           ["B 0 0 1", "B 1 0 1", "S 0 2 3", "B 2 0 0", "S 2 4 7", "E 2", "S 4 8 3", "E 0", "S 8 10 2", "B 2 1 0",
                                            "S 10 16 6", "E 1", "E 2"]),
    "a_first_row_before_the_buffer_never_starts": (([(0, 16, 1)], [], []), ["S 3 16 0"]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_the_walk_makes_the_hand_written_segments(harness, name):
    (notes, ratio, mult), want = HAND[name]
    span = (3, 16) if name.startswith("a_first_row_before") else (0, 16)
    assert _run(harness, _input(_hand(notes, ratio, mult), span))[1:] == want


def test_a_count_above_the_tables_rows_is_clamped(harness):
    """count = 5 in tables of 2 rows: the walk stops after the second row; ASan would see a third read"""
    tbs = _hand([(0, 4, 1), (4, 8, 0)], [(0, 8, 1)], [])
    tbs[0]["count"][0] = 5
    out = _run(harness, _input(tbs, (0, 16), K=2))
    assert out[1:] == ["B 0 0 1", "B 1 0 1", "S 0 4 3", "E 0", "B 0 1 0", "S 4 8 3", "E 0", "E 1", "S 8 16 0"]


def test_the_voices_state_layout_under_the_sanitizers(tmp_path):
    run_sanitized(os.path.join(ROOT, "tests", "cpp", "pmctl_state_host.cpp"), tmp_path)
