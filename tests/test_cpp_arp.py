"""CPU: the arpeggiator stage's lane steps (zang_amd/csrc/arp_lane.hip.h, the text k_arp_schedule runs) compiled for the host with
ASan and UBSan into a stand-alone program (tests/cpp/arp_lane_host.cpp) and run over the case list: the tables, counts, dropped
rows and state it prints after each of the six buffers are the model's (tests/arp_reference.py).  No sanitizer enters Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import arp_cases as ac
from tests import arp_reference as ar
from tests.hostprog import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "arp_lane_host.cpp")
PLAYERS = 66


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_sanitized(SRC, tmp_path_factory.mktemp("arp_lane"))


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def _input(case, rec, n):
    lines = [f"{_bits(case.sample_rate)} {case.n_keys} {ac.OUT_LEN} {case.max_spans} {n} {ac.BUFFERS} {ac.OUTER_SPANS}",
             " ".join(str(_bits(f)) for f in case.key_freqs())]
    for b in range(ac.BUFFERS):
        for p in range(n):
            outer = rec.outer[b][p]
            row = [str(len(outer))]
            for s, e, held, _ in outer:
                m = ac.mask_of(held)
                row += [str(s), str(e), str(m & 0xffffffff), str(m >> 32)]
            lines.append(" ".join(row))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("case", ac.CASES, ids=ac.CASE_IDS)
def test_the_lane_equals_the_model_after_every_buffer(harness, case):
    rec = ac.run(case)
    out = _run(harness, _input(case, rec, PLAYERS))
    assert out[0] == f"nd {case.note_duration}" and out[-2] == "PASS", out[:2]
    i = 1
    for b in range(ac.BUFFERS):
        ref, dropped = ar.table(rec.inner[b][:PLAYERS], case.max_spans)
        assert out[i] == f"B {b} dropped {dropped}", (b, out[i])
        i += 1
        for p in range(PLAYERS):
            head = [int(x) for x in out[i].split()[1:]]
            assert out[i].startswith("P ") and head == [int(ref["count"][p])] + rec.words[b][p], (b, p, out[i], rec.words[b][p])
            i += 1
            for k in range(head[0]):
                want = [int(ref["start"][k, p]), int(ref["end"][k, p]), _bits(ref["freq"][k, p]), int(ref["note_on"][k, p]), int(ref["nic"][k, p])]
                assert out[i].startswith("R ") and [int(x) for x in out[i].split()[1:]] == want, (b, p, k, out[i], want)
                i += 1


@pytest.mark.parametrize("rate", ac.REJECTED_RATES, ids=[str(r) for r in ac.REJECTED_RATES])
def test_rejected_rates(harness, rate):
    assert _run(harness, f"{_bits(rate)} 1 256 4 1 0 4\n0\n")[0] == "invalid"
