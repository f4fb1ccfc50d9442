"""zang::LiveVoiceBank (include/zang_hip.hpp) from a compiled host: tests/cpp/live_bank_host.cpp compiles and links here (CPU) and on a
GPU checks the live bank's tables against the host classes composed per instrument, a paint from its view against an uploaded table, and
a state saved in the middle of the stream restored into a second bank, without Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "live_bank_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "live_bank_host")


def _build():
    import zang_amd  # noqa: F401  (fails loudly if libzang_hip.so is missing)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "zang_amd"), "-lzang_hip", "-Wl,-rpath," + os.path.join(ROOT, "zang_amd"),
                           "-L" + rocm + "/lib", "-Wl,-rpath," + rocm + "/lib", "-o", EXE])


def test_live_bank_host_program_compiles_and_links():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_live_bank_host_program():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    assert "identical" in r.stdout and "bit-exact" in r.stdout and "state restored" in r.stdout
