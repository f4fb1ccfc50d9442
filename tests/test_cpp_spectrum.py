"""zang::Spectrum, zang::Spectrogram and zang::fft (include/zang_hip.hpp) from a compiled host: tests/cpp/spectrum_host.cpp compiles
and links here (CPU); on a GPU it plots a fixed 66-voice image and prints one checksum word per result, which must be the words of
the yardstick (tests/spectrum_reference.py) on the same image."""
import os
import subprocess

import numpy as np
import pytest

from tests import spectrum_reference as sr
from tests.hostprog import FNV_BASIS, build_linked, fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "spectrum_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "spectrum_host")
V, F, W, H = 66, 1024 + 8, 3, 5


def test_spectrum_host_program_compiles_and_links():
    build_linked(SRC, EXE)
    assert os.path.exists(EXE)


def _image():
    """[frame][voice], the program's pattern: every value k / 128 - 1, exact in f32"""
    v = np.arange(V, dtype=np.int64)[None, :]
    f = np.arange(F, dtype=np.int64)[:, None]
    return (((v * 131 + f * 71 + (f * f) % 29) % 257).astype(np.float32) / np.float32(128.0) - np.float32(1.0)).astype(np.float32)


def expected_words(oracle):
    img = _image()
    words = ["plot %016x" % fnv1a(FNV_BASIS, np.ascontiguousarray(sr.plot(img[3:3 + 1024]).T).tobytes())]
    gram = sr.Spectrogram(V, W, H, sr.oracle_pow10(oracle))
    for b, log in enumerate([False, False, True, True, True]):
        gram.plot(img[2 * b:2 * b + 1024], log)
        h = fnv1a(FNV_BASIS, np.ascontiguousarray(gram.buffer).tobytes())
        words.append("gram %d %d %016x" % (b, gram.drawindex, fnv1a(h, np.ascontiguousarray(gram.scrolled()).tobytes())))
    host = np.ascontiguousarray(img.T).reshape(-1)                     # the program's [voice][frame] array
    re = np.ascontiguousarray(host[:V * 64].reshape(V, 64).T)
    im = np.ascontiguousarray(host[V * 64:2 * V * 64].reshape(V, 64).T)
    r, i = np.ascontiguousarray(re[7:39]), np.ascontiguousarray(im[7:39])
    sr.fft(32, r, i)
    re[7:39], im[7:39] = r, i
    words.append("fft %016x" % fnv1a(fnv1a(FNV_BASIS, np.ascontiguousarray(re.T).tobytes()), np.ascontiguousarray(im.T).tobytes()))
    return words


def test_the_expected_words_need_no_device(oracle):
    """the yardstick's side alone: the image is the program's pattern, the state machine wraps and clears where the program's does"""
    img = _image()
    assert img[5, 7] == np.float32(((7 * 131 + 5 * 71 + 25) % 257) / 128.0 - 1.0) and np.abs(img).max() <= 1.0
    words = expected_words(oracle)
    assert [w.split()[0] for w in words] == ["plot"] + ["gram"] * 5 + ["fft"]
    assert [w.split()[2] for w in words[1:6]] == ["1", "2", "1", "2", "0"]          # drawindex: the flip at the third plot resets it
    assert len(set(words)) == 7


@pytest.mark.gpu
def test_spectrum_host_program_prints_the_yardsticks_words(ctx, oracle):
    build_linked(SRC, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    assert r.stdout.split("\n")[:7] == expected_words(oracle), r.stdout
