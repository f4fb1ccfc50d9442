"""GPU: zang_amd.fmsynth.FMSynth -- N of the reference's FM synthesizers (examples/example_fmsynth.zig MainModule, :358-520) with
no host work per voice -- against MainModule composed on the host (tests/fm_reference.py MainModuleRef: the host classes of
zang_amd/notes.py, the oracle's SineOsc LFOs, the FM helper), synth by synth and bit for bit: 9 synths x polyphony 8 (72 voices, a
group straddling the wave edge), six buffers of 1,024 frames, pushed impulses."""
import ctypes as C

import numpy as np
import pytest

from tests import fm_reference as fr
from tests.util import assert_bitexact

pytestmark = pytest.mark.gpu
N, P, F, B, SR = 9, 8, 1024, 6, 48000.0
SILENT = 4                                       # a synth that nobody plays
FRAMES = (0, 300, 640)                           # the impulses' frames: few distinct sub-spans for the helper's sequential loop


def _events():
    """per buffer a list of (synth, frame, note_id, freq, note_on) in push order"""
    rng = np.random.default_rng(20261018)
    out, next_id, held = [], 1, {j: [] for j in range(N)}
    for b in range(B):
        ev = []
        for j in range(N):
            if j == SILENT:
                continue
            if j == 2 and b == 1:                # more than 8 simultaneous notes on one synth: voices are stolen
                for k in range(11):
                    ev.append((j, 0, next_id, 110.0 * (k + 2), True)); held[j].append(next_id); next_id += 1
                continue
            if j == 6 and b == 2:                # 33 pushes into one buffer: the queue takes 32
                for k in range(33):
                    on = k % 3 != 2 or not held[j]
                    nid = next_id if on else held[j].pop(0)
                    ev.append((j, FRAMES[min(k // 11, 2)], nid, 55.0 * (k % 12 + 2), on))
                    if on:
                        held[j].append(next_id); next_id += 1
                continue
            for f in FRAMES:
                u = rng.random()
                if u < 0.45:                     # a key goes down
                    ev.append((j, f, next_id, float(np.float32(rng.uniform(80.0, 1200.0))), True)); held[j].append(next_id); next_id += 1
                elif u < 0.75 and held[j]:       # a key comes up
                    ev.append((j, f, held[j].pop(int(rng.integers(0, len(held[j])))), 440.0, False))
        out.append(ev)
    return out


def _mixed_patches():
    pats = [list(fr.DEFAULT_PATCH) for _ in range(N)]
    for j in (1, 2, 6, 8):                       # algorithm 0 on some synths, with something to hear from the modulator
        pats[j][fr.ALGORITHM] = 0
        pats[j][fr.MOD_FEEDBACK] = j % 8
        pats[j][fr.CAR_WAVEFORM] = j % 4
    pats[3][fr.MOD_TREMOLO], pats[3][fr.CAR_VIBRATO], pats[3][fr.MOD_WAVEFORM] = 1, 1, 3
    for p in pats:                               # 2 ms attack and decay: the six buffers see every envelope stage
        p[fr.MOD_ATTACK] = p[fr.CAR_ATTACK] = p[fr.CAR_DECAY] = 15
    return pats


@pytest.mark.parametrize("patches", ["default", "mixed"])
def test_fmsynth_equals_the_host_main_module(ctx, patches, oracle):
    from zang_amd.fmsynth import FMSynth
    pats = None if patches == "default" else _mixed_patches()
    synth = FMSynth(ctx, N, pats, polyphony=P, sample_rate=SR, max_impulses=64)
    twin = FMSynth(ctx, N, pats, polyphony=P, sample_rate=SR, max_impulses=64)           # the same events through paint_pcm
    assert synth.split == (patches == "mixed")
    ref = fr.MainModuleRef(N, pats, P, SR)
    L = oracle.lib()
    loudest = 0.0
    for b, ev in enumerate(_events()):
        for j, f, nid, freq, on in ev:
            synth.push(j, f, nid, freq, on); twin.push(j, f, nid, freq, on); ref.push(j, f, nid, freq, on)
        rows = synth.paint(F)
        pcm = twin.paint_pcm(F, 0.25)
        ctx.sync()
        want = ref.paint(F)
        got = rows.cpu().numpy()
        for j in range(N):
            assert_bitexact(got[j], want[j], f"buffer {b}, synth {j}")
        assert not want[SILENT].any()
        bytes_want = np.zeros((N, F * 2), np.uint8)
        for j in range(N):
            L.zo_mixdown_s16lsb(bytes_want[j].ctypes.data_as(C.POINTER(C.c_uint8)), oracle.fptr(np.ascontiguousarray(want[j])), F, 1, 0, 0.25)
        assert np.array_equal(pcm.cpu().numpy(), bytes_want), f"buffer {b}: pcm"
        loudest = max(loudest, float(np.abs(want).max()))
    assert loudest > 0.05
    assert synth.overflows() == 0 and twin.overflows() == 0
    assert ref.max_spans >= 3
    synth.close(); twin.close()
