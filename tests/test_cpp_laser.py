"""zang::SfxKit and zang::Laser (include/zang_hip.hpp) from a compiled host: tests/cpp/laser_host.cpp compiles and links here
(CPU); on a GPU it paints one small span case and prints a checksum of the images' and the state's bits, which must be the
checksum of the same paints made through ctypes.  And the effect kit's packing under AddressSanitizer + UBSan, as a stand-alone
program with its own main (tests/cpp/sfx_kit_host.cpp): nothing loaded into python runs under a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest
from tests.hostprog import build_linked, fnv1a, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "laser_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "laser_host")
KIT_SRC = os.path.join(ROOT, "tests", "cpp", "sfx_kit_host.cpp")


def test_laser_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


def test_kit_packing_under_the_sanitizers(tmp_path):
    """three kits (empty curves, one effect, five effects of unequal lengths) packed into a heap block of exactly the library's
    size, descriptors and nodes read back; the refusals of zh_sfx_kit_create"""
    run_sanitized(KIT_SRC, tmp_path)


@pytest.mark.gpu
def test_laser_host_program_paints_what_ctypes_paints(ctx):
    from tests.util import from_image
    from zang_amd import modules as mod, sfx, zang
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    theirs = int(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1), 16)
    V, K, F, S, E = 66, 2, 64, 3, 60
    ramp = [(0.0, 300.0), (0.001, 900.0)]
    kit = sfx.SfxKit(ctx, [sfx.default_effect(), ((ramp, sfx.linear), (ramp, sfx.smoothstep), ([(0.0, 1.0), (0.001, 0.0)], sfx.linear))])
    v = np.arange(V)
    k = np.arange(K)[:, None]
    start = np.stack([S + v % 5, 30 + v % 7]); end = np.stack([np.full(V, 30), np.full(V, E)])
    nic = np.stack([v % 2, (v // 2) % 2])
    m = mod.Laser(V, ctx)
    table = m.span_table(v % 3, start, end, nic, {"freq_mul": ((0.875 + 0.125 * ((v + k) % 3)).astype(np.float32), None),
                                                  "effect": (None, (v + k) % 3)})
    img = ctx.image(F, V, fill=0.0)
    p = m.Params(kit, 48000.0, 1.0, 2.0, 0.5, 0.5, 0)
    m.paint_spans(zang.Span(S, E), [img], None, p, table)
    ctx.sync()
    first = from_image(img).tobytes()
    m.paint_spans(zang.Span(S, E), [img], None, p, table, zero_first=True)
    m.paint(zang.Span(S, E), [img], [], False, p)
    ctx.sync()
    ours = fnv1a(fnv1a(fnv1a(0xCBF29CE484222325, first), from_image(img).tobytes()), m.state().tobytes())
    assert ours == theirs, (hex(ours), hex(theirs))
    m.close(); kit.close()
