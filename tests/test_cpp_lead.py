"""zang::Porta and zang::Vibrato (include/zang_hip.hpp) from a compiled host: tests/cpp/lead_host.cpp compiles and links here (CPU);
on a GPU it paints one small span case per voice and prints a checksum of the images' and the state's bits, which must be the
checksum of the same paints made through ctypes."""
import os
import re
import subprocess

import numpy as np
import pytest
from tests.hostprog import build_linked, fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lead_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "lead_host")


def test_lead_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_lead_host_program_paints_what_ctypes_paints(ctx):
    from tests.util import from_image
    from zang_amd import modules as mod, zang
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    V, K, F, S, E = 66, 2, 64, 3, 60
    v = np.arange(V)
    k = np.arange(K)[:, None]
    start = np.stack([S + v % 5, 30 + v % 7]); end = np.stack([np.full(V, 30), np.full(V, E)])
    nic = np.stack([np.ones(V, np.int64), (v // 2) % 2])
    f32 = np.float32
    fr = lambda n: float(f32(n) / f32(48000.0))
    for name, cls, patch in (("porta", mod.Porta, mod.Porta.Patch(glide=fr(30.0), attack=fr(15.0), decay=fr(25.0), release=fr(40.0))),
                             ("vibrato", mod.Vibrato, mod.Vibrato.Patch(vib_hz=400.0, depth=0.3, color=0.3))):
        theirs = int(re.search(name + r" checksum ([0-9a-f]{16})", r.stdout).group(1), 16)
        m = cls(V, ctx)
        table = m.span_table(v % 3, start, end, nic, {"freq": ((110.0 * (1 + (v + k) % 5)).astype(np.float32), None),
                                                      "note_on": (None, ((k == 0) | (v % 4 != 0)).astype(np.uint32))})
        img, sync = ctx.image(F, V, fill=0.0), ctx.image(F, V, fill=0.0)
        p = m.Params(48000.0, 220.0, True, patch)
        m.paint_spans(zang.Span(S, E), [img, sync], None, p, table)
        ctx.sync()
        first = from_image(img).tobytes()
        m.paint_spans(zang.Span(S, E), [img, sync], None, p, table, zero_first=True)
        m.paint(zang.Span(S, E), [img], [], False, p)
        ctx.sync()
        h = fnv1a(fnv1a(fnv1a(0xCBF29CE484222325, first), from_image(img).tobytes()), from_image(sync).tobytes())
        ours = fnv1a(h, m.state().tobytes())
        assert ours == theirs, (name, hex(ours), hex(theirs))
        m.close()
