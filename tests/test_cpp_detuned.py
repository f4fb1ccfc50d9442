"""zang::Detuned (include/zang_hip.hpp) from a compiled host: tests/cpp/detuned_host.cpp compiles and links here (CPU); on a GPU
it paints one small span case and prints a checksum of the images' and the state's bits, which must be the checksum of the same
paints made through ctypes.  And the state layout (struct <-> [word][voice] rows, csrc/detuned.hip.h) under AddressSanitizer +
UBSan, as a stand-alone program with its own main (tests/cpp/detuned_state_host.cpp): nothing loaded into python runs under a
sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest
from tests.hostprog import build_linked, fnv1a, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "detuned_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "detuned_host")
STATE_SRC = os.path.join(ROOT, "tests", "cpp", "detuned_state_host.cpp")


def test_detuned_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


def test_state_layout_under_the_sanitizers(tmp_path):
    """0, 1, 65 and 130 voices packed into a heap block of exactly the library's size and read back: every word written once, at
    [word][voice]; every field of zh_detuned_state back on bits, the taps as zeros"""
    run_sanitized(STATE_SRC, tmp_path)


@pytest.mark.gpu
def test_detuned_host_program_paints_what_ctypes_paints(ctx):
    from tests.util import from_image
    from zang_amd import modules as mod, zang
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    theirs = int(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1), 16)
    V, K, F, S, E = 66, 2, 64, 3, 60
    v = np.arange(V)
    k = np.arange(K)[:, None]
    start = np.stack([S + v % 5, 30 + v % 7]); end = np.stack([np.full(V, 30), np.full(V, E)])
    nic = np.stack([np.ones(V, np.int64), (v // 2) % 2])
    m = mod.Detuned(V, ctx, 1000)
    table = m.span_table(v % 3, start, end, nic, {"freq": ((110.0 * (1 + (v + k) % 5)).astype(np.float32), None),
                                                  "note_on": (None, ((k == 0) | (v % 4 != 0)).astype(np.uint32)),
                                                  "mode": (None, ((v + k) % 4).astype(np.uint32))})
    img, sync = ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)
    f32 = np.float32
    patch = m.Patch(warble_hz=400.0, attack=float(f32(15.0) / f32(48000.0)), decay=float(f32(25.0) / f32(48000.0)),
                    release=float(f32(40.0) / f32(48000.0)), res=0.3)
    p = m.Params(48000.0, 220.0, True, 0, patch)
    m.paint_spans(zang.Span(S, E), [img, sync], None, p, table)
    ctx.sync()
    first = from_image(img).tobytes()
    m.paint_spans(zang.Span(S, E), [img, sync], None, p, table, zero_first=True)
    m.paint(zang.Span(S, E), [img], [], False, p)
    ctx.sync()
    h = fnv1a(fnv1a(fnv1a(0xCBF29CE484222325, first), from_image(img).tobytes()), from_image(sync).tobytes())
    ours = fnv1a(h, m.state().tobytes())
    assert ours == theirs, (hex(ours), hex(theirs))
    m.close()
