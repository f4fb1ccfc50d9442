"""CPU: what the HardSquare GPU tests take for granted about their reference and their inputs -- the oracle alone."""
import numpy as np
import pytest

from tests import hard_square_cases as hq
from tests import lead_cases as lc


def test_the_gate_off_multiply_add_is_still_performed(oracle):
    """note_on clear over an image of -0.0: inside the sub-span osc * 0.0f is ADDED, so -0.0 becomes +0.0 (the square's -1 times
    +0 gives -0.0, whose sum with -0.0 stays -0.0: both show); outside nothing changes; the oscillator's phase still advances"""
    vs = hq.voices(oracle, 1)
    img = np.full((1, 256), -0.0, np.float32)
    hq.reference_plain(oracle, vs, 8, 240, img, None, hq.SR, 440.0, False)
    bits = img.view(np.uint32)[0]
    assert (bits[:8] == 0x80000000).all() and (bits[240:] == 0x80000000).all()
    assert set(bits[8:240].tolist()) == {0, 0x80000000} and vs[0].cnt != 0


def test_the_oracle_alone_stays_under_the_nan_cap_for_the_hostile_inputs(oracle):
    V, tb = lc.hostile_freq_tables()
    vs = hq.voices(oracle, V)
    ref, rsync = lc.base_image(V, 90), lc.base_image(V, 91)
    hq.reference_spans(oracle, vs, tb, ref, rsync, False)
    assert 0.0 < lc.worst_row_nan_share(ref, rsync) <= hq.NAN_CAP
    for sr in lc.HOSTILE_SR:
        vs = hq.voices(oracle, 65)
        ref, rsync = lc.base_image(65, 900), lc.base_image(65, 910)
        freq = np.random.default_rng(17).uniform(110.0, 880.0, 65).astype(np.float32)
        hq.reference_plain(oracle, vs, lc.SPAN[0], lc.HOSTILE_FROM, ref, rsync, hq.SR, freq, True)
        hq.reference_plain(oracle, vs, lc.HOSTILE_FROM, lc.SPAN[1], ref, rsync, sr, freq, True)
        assert lc.worst_row_nan_share(ref, rsync) <= hq.NAN_CAP, sr
