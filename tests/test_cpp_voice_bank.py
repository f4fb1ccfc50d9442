"""zang::VoiceBank (include/zang_hip.hpp) from a compiled host: tests/cpp/voice_bank_host.cpp compiles and links here (CPU) and on
a GPU checks the bank's tables against zh_poly_voice_schedule and two paints from its views against uploaded tables, without Python."""
import os
import subprocess

import pytest
from tests.hostprog import build_linked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "voice_bank_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "voice_bank_host")


def test_voice_bank_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_voice_bank_host_program():
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    assert "identical" in r.stdout and "bit-exact" in r.stdout
