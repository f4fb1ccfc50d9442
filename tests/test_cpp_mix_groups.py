"""zang::mixdownGroups / mixdownGroupsPcm (include/zang_hip.hpp) from a compiled host: tests/cpp/mix_groups_host.cpp compiles and
links here (CPU) and on a GPU checks both calls against a plain C++ loop and against the per-group calls they replace, without Python."""
import os
import subprocess

import pytest
from tests.hostprog import build_linked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mix_groups_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "mix_groups_host")


def test_mix_groups_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_mix_groups_host_program():
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    assert "bit-exact" in r.stdout and "identical" in r.stdout
