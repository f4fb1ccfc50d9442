"""CPU: the state layouts of the ten builtin modules that share one host side (zang_amd/csrc/state_block.hip.h over the Layouts
of module_state.hip.h and fm.hip.h) under AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/module_state_host.cpp): nothing loaded into python runs under a sanitizer."""
import os

from tests.hostprog import run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "module_state_host.cpp")


def test_module_state_layouts_under_the_sanitizers(tmp_path):
    """n = 0, 1, 65, 130: hostile structs -> rows in a heap block of exactly kWords * n words -> structs, bit for bit; every word
    written; the rows the kernels read hold voice v at column v; kWords and sizeof(State) are the numbers of the code they replaced"""
    run_sanitized(SRC, tmp_path)
