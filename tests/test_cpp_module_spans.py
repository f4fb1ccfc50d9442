"""The builtin modules' span paints from a compiled C++ host (include/zang_hip.hpp mod::X::paint_spans): compiles here (CPU);
on a GPU tests/cpp/module_spans_host.cpp paints a PulseOsc and a Sampler voice bank over one per-voice sub-span table and
checks them bit for bit against the oracle's per-sub-span paints."""
import os
import subprocess

import pytest

from tests.test_cpp_host import ROOT, _build

SRC = os.path.join(ROOT, "tests", "cpp", "module_spans_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "module_spans_host")


def test_cpp_module_spans_host_compiles_and_links():
    _build(SRC, EXE)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_module_spans_host_program():
    _build(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS") and r.stdout.count("bit-exact") == 2, r.stdout
