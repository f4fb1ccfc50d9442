"""CPU: the state layouts of the ten builtin modules that share one host side (zang_amd/csrc/state_block.hip.h over the Layouts
of module_state.hip.h and fm.hip.h) under AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/module_state_host.cpp): nothing loaded into python runs under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "module_state_host.cpp")


def test_module_state_layouts_under_the_sanitizers(tmp_path):
    """n = 0, 1, 65, 130: hostile structs -> rows in a heap block of exactly kWords * n words -> structs, bit for bit; every word
    written; the rows the kernels read hold voice v at column v; kWords and sizeof(State) are the numbers of the code they replaced"""
    exe = str(tmp_path / "module_state_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-4000:]
