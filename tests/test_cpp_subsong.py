"""CPU: the subsong stage's lane steps (zang_amd/csrc/subsong_lane.hip.h, the text k_subsong_schedule runs) compiled for the host
with ASan and UBSan into a stand-alone program (tests/cpp/subsong_lane_host.cpp) and run over the case list: the tables, counts,
dropped rows and state it prints after each of the six buffers are the model's (tests/subsong_reference.py).  No sanitizer enters
Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import subsong_cases as sc
from tests import subsong_reference as sr
from tests.hostprog import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "subsong_lane_host.cpp")
PLAYERS = 66


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("subsong_lane"), ["-ffp-contract=off"])


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def _head(kit, max_spans, n, buffers, in_spans=sc.OUTER_SPANS):
    events = [e for m in kit for e in m]
    offsets = np.cumsum([0] + [len(m) for m in kit])
    lines = [f"{sr.bits(sc.BASE_FREQ)} {sc.OUT_LEN} {max_spans} {n} {buffers} {in_spans} {len(kit)} {len(events)}",
             " ".join(str(int(o)) for o in offsets)]
    lines += [f"{sr.bits(t)} {i} {sr.bits(f)} {int(on)}" for t, i, f, on in events]
    return lines


def _outer_row(outer):
    row = [str(len(outer))]
    for s, e, (freq, on, melody), changed in outer:
        row += [str(s), str(e), str(int(changed)), str(sr.bits(freq)), str(int(on)), str(melody)]
    return " ".join(row)


def _input(case, rec, n):
    lines = _head(sc.KIT, case.max_spans, n, sc.BUFFERS)
    for b in range(sc.BUFFERS):
        lines.append(str(sr.bits(case.rate(b))))
        lines += [_outer_row(rec.outer[b][p]) for p in range(n)]
    return "\n".join(lines) + "\n"


def _check_buffer(out, i, b, inner, words, max_spans):
    """the harness's lines from i on are buffer b's: -> the index after them"""
    n = len(inner)
    ref, dropped = sr.table(inner, max_spans)
    assert out[i] == f"B {b} dropped {dropped}", (b, out[i])
    i += 1
    for p in range(n):
        head = [int(x) for x in out[i].split()[1:]]
        assert out[i].startswith("P ") and head == [int(ref["count"][p])] + words[p], (b, p, out[i], words[p])
        i += 1
        for k in range(head[0]):
            want = [int(ref["start"][k, p]), int(ref["end"][k, p]), sr.bits(ref["freq"][k, p]), int(ref["note_on"][k, p]), int(ref["nic"][k, p])]
            assert out[i].startswith("R ") and [int(x) for x in out[i].split()[1:]] == want, (b, p, k, out[i], want)
            i += 1
    return i


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_the_lane_equals_the_model_after_every_buffer(harness, case):
    rec = sc.run(case)
    out = _run(harness, _input(case, rec, PLAYERS))
    assert out[-2] == "PASS", out[-3:]
    i = 0
    for b in range(sc.BUFFERS):
        i = _check_buffer(out, i, b, rec.inner[b][:PLAYERS], rec.words[b][:PLAYERS], case.max_spans)


def test_an_impossible_outer_sub_span_ends_the_list(harness):
    """end <= start, or end above out_len: the rows before it are painted, nothing after it, and the state stops there"""
    kf = sc.key_freq(0)
    for bad in ((100, 100), (120, 100), (100, sc.OUT_LEN + 1)):
        rows = [(0, 100, (kf, True, sc.M_REF), True), (bad[0], bad[1], (kf, True, sc.M_PAIRS), True), (100, 256, (kf, True, sc.M_PAIRS), True)]
        model = sr.SubtrackPlayer(sc.KIT, sc.BASE_FREQ)
        inner = model.paint(0, 100, True, sc.RATE, kf, True, sc.M_REF)
        text = "\n".join(_head(sc.KIT, 8, 1, 1) + [str(sr.bits(sc.RATE)), _outer_row(rows)]) + "\n"
        out = _run(harness, text)
        assert _check_buffer(out, 0, 0, [inner], [model.words()], 8) == len(out) - 2 and out[-2] == "PASS"


def test_an_empty_kit_plays_nothing(harness):
    """K = 0: init() latches no melody, every press plays an empty song"""
    kf = sc.key_freq(0)
    rows = [(0, 256, (kf, True, 0), True)]
    model = sr.SubtrackPlayer([], sc.BASE_FREQ)
    assert model.words()[2] == sr.NO_MELODY
    inner = model.paint(0, 256, True, sc.RATE, kf, True, 0)
    assert inner == []
    out = _run(harness, "\n".join(_head([], 8, 1, 1) + [str(sr.bits(sc.RATE)), _outer_row(rows)]) + "\n")
    assert _check_buffer(out, 0, 0, [inner], [model.words()], 8) == len(out) - 2
