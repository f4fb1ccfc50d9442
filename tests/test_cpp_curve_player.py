"""zang::CurvePlayer (include/zang_hip.hpp) from a compiled host: tests/cpp/curve_player_host.cpp compiles and links here (CPU);
on a GPU it paints one small span case and prints a checksum of both images' and the state's bits, which must be the checksum of
the same paints made through ctypes.  And the state layout (struct <-> [word][voice] rows, csrc/curve_player.hip.h) under
AddressSanitizer + UBSan, as a stand-alone program with its own main (tests/cpp/curve_player_state_host.cpp): nothing loaded into
python runs under a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest
from tests.hostprog import build_linked, fnv1a, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "curve_player_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "curve_player_host")
STATE_SRC = os.path.join(ROOT, "tests", "cpp", "curve_player_state_host.cpp")


def test_curve_player_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


def test_state_layout_under_the_sanitizers(tmp_path):
    """1, 3 and 65 voices packed into a heap block of exactly the library's size and read back: every word written once, at
    [word][voice] in the struct's own order; every field of zh_curve_player_state back on bits"""
    run_sanitized(STATE_SRC, tmp_path)


@pytest.mark.gpu
def test_curve_player_host_program_paints_what_ctypes_paints(ctx):
    from tests.util import from_image
    from zang_amd import modules as mod, sfx, zang
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    theirs = int(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1), 16)
    V, K, F, S, E = 66, 2, 64, 3, 60
    kit = sfx.SfxKit(ctx, [sfx.curve_example_effect(),
                           (([(0.0, 300.0), (0.001, 900.0)], sfx.linear), ([(0.0, 2000.0), (0.0005, 500.0)], sfx.smoothstep), ([], sfx.linear))])
    v = np.arange(V)
    k = np.arange(K)[:, None]
    start = np.stack([S + v % 5, 30 + v % 7]); end = np.stack([np.full(V, 30), np.full(V, E)])
    nic = np.stack([v % 2, (v // 2) % 2])
    m = mod.CurveVoice(V, ctx)
    table = m.span_table(v % 3, start, end, nic, {"rel_freq": ((0.75 + 0.25 * ((v + k) % 3)).astype(np.float32), None),
                                                  "effect": (None, (v + k) % 3)})
    img, sync = ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)
    p = m.Params(kit, 48000.0, 1.5, 0)
    m.paint_spans(zang.Span(S, E), [img, sync], None, p, table)
    ctx.sync()
    first = from_image(img).tobytes(), from_image(sync).tobytes()
    m.paint_spans(zang.Span(S, E), [img, sync], None, p, table, zero_first=True)
    m.paint(zang.Span(S, E), [img, sync], [], False, p)
    ctx.sync()
    ours = 0xCBF29CE484222325
    for data in (*first, from_image(img).tobytes(), from_image(sync).tobytes(), m.state().tobytes()):
        ours = fnv1a(ours, data)
    assert ours == theirs, (hex(ours), hex(theirs))
    m.close(); kit.close()
