"""zang::FMInstrument (include/zang_hip.hpp) from a compiled host: tests/cpp/fm_host.cpp compiles and links here (CPU); on a GPU
it paints 130 voices over two spans and prints a checksum of the image's and the state's bits, which must be the checksum of the
same paints made through ctypes."""
import os
import re
import subprocess

import numpy as np
import pytest
from tests.hostprog import build_linked, fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fm_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "fm_host")


def test_fm_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_fm_host_program_paints_what_ctypes_paints(ctx):
    from tests.util import dev, from_image, to_image
    from zang_amd import abi, modules as mod, zang
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    theirs = int(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1), 16)
    V, G, F, sr = 130, 5, 1024, 48000.0
    NI = V // G
    pats = np.tile(np.array(mod.FMInstrument.default_patch(), np.uint32), (NI, 1))
    j = np.arange(NI)
    pats[:, abi.FM_MOD_FEEDBACK], pats[:, abi.FM_ALGORITHM], pats[:, abi.FM_CAR_WAVEFORM] = j % 8, j % 2, j % 4
    pats[:, abi.FM_MOD_ATTACK] = pats[:, abi.FM_CAR_ATTACK] = 15
    pats[:, abi.FM_CAR_TREMOLO] = pats[:, abi.FM_MOD_VIBRATO] = (j // 2) % 2
    f = np.arange(F)
    trem = (((f[None, :] * 7 + j[:, None] * 3) % 101).astype(np.float32) / np.float32(101.0) - np.float32(0.5)).astype(np.float32)
    vib = (((f[None, :] * 5 + j[:, None] * 11) % 89).astype(np.float32) / np.float32(89.0) - np.float32(0.5)).astype(np.float32)
    freq = (np.float32(55.0) + np.float32(13.0) * np.arange(V, dtype=np.float32)).astype(np.float32)
    m = mod.FMInstrument(V, ctx, group=G)
    m.set_patches(pats)
    img = ctx.image(F, V, fill=0.0)
    ti, vi = to_image(trem), to_image(vib)
    m.paint(zang.Span(0, 200), [img], None, True, m.Params(sr, ti, vi, dev(freq), True))
    m.paint(zang.Span(200, F), [img], None, False, m.Params(sr, ti, vi, dev(freq), False))
    ctx.sync()
    ours = fnv1a(fnv1a(0xCBF29CE484222325, from_image(img).tobytes()), m.state().tobytes())
    assert ours == theirs, (hex(ours), hex(theirs))
    m.close()
