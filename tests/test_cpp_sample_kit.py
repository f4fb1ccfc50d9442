"""zang::SampleKit and mod::paintKitSpans (include/zang_hip.hpp) from a compiled host: tests/cpp/sample_kit_host.cpp compiles and
links here (CPU); on a GPU it paints one small kit span case twice and prints a checksum of the images' and the state's bits, which
must be the checksum of the same paints made through ctypes."""
import os
import re
import subprocess

import numpy as np
import pytest
from tests.hostprog import build_linked, fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sample_kit_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "sample_kit_host")


def test_sample_kit_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_sample_kit_host_program_paints_what_ctypes_paints(ctx):
    from tests.util import from_image
    from zang_amd import modules as mod, zang
    from zang_amd.samplekit import SampleKit
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    theirs = int(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1), 16)
    V, K, F, S, E = 66, 2, 64, 3, 60
    lens, chans, rates = (37, 200, 125), (1, 2, 1), (44100, 22050, 48000)
    kit = SampleKit(ctx, [(chans[j], rates[j], j, ((np.arange(lens[j]) * 37 + j * 101 + 13) % 256).astype(np.uint8)) for j in range(3)])
    v = np.arange(V)
    k = np.arange(K)[:, None]
    start = np.stack([S + v % 5, 30 + v % 7]); end = np.stack([np.full(V, 30), np.full(V, E)])
    nic = np.stack([v % 2, (v // 2) % 2])
    rs = np.array([44100.0, 22050.5, -30000.0, 48000.0], np.float32)
    m = mod.Sampler(V, ctx)
    table = m.kit_span_table(v % 3, start, end, nic, {"sample_rate": (rs[(v + 2 * k) % 4], None), "loop": (None, (v + k) % 2),
                                                      "sample": (None, (v + k) % 4), "channel": (None, (v + k) % 2)})
    img = ctx.image(F, V, fill=0.0)
    p = m.KitParams(kit, 44100.0, 0, 0, False)
    m.paint_kit_spans(zang.Span(S, E), [img], None, p, table)
    ctx.sync()
    first = from_image(img).tobytes()
    m.paint_kit_spans(zang.Span(S, E), [img], None, p, table, zero_first=True)
    ctx.sync()
    ours = fnv1a(fnv1a(fnv1a(0xCBF29CE484222325, first), from_image(img).tobytes()), m.state().tobytes())
    assert ours == theirs, (hex(ours), hex(theirs))
    m.close(); kit.close()
