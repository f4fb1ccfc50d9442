"""GPU: DetunedPlayer (zang_amd/detuned.py) -- N of examples/example_detuned.zig's MainModule played live from pushed impulses --
against MainModule composed on the host (tests/detuned_reference.py: ImpulseQueue -> Trigger from zang_amd/notes.py,
OuterInstrument.paint as oracle calls per sub-span, the bypass, StereoEchoes from the oracle's delay calls).  Everything on bits."""
import numpy as np
import pytest

from tests import detuned_cases as dc
from tests import detuned_reference as dr
from tests import util

pytestmark = pytest.mark.gpu
F, B, N, MAIN_DELAY = 256, 6, 3, 300


def _pushes():
    """per buffer (player, frame, note_id, freq, note_on) in push order, as keyEvent pushes them (a note-off only for the held
    key): two at one frame, a note-off, a new key while one is held; player 2 is pushed to once, late"""
    return [[(0, 0, 1, 220.0, True), (1, 17, 2, 330.0, True)],
            [(0, 40, 3, 440.0, True), (0, 40, 4, 110.0, True), (1, 200, 2, 330.0, False)],          # two at one frame; player 1 releases
            [(1, 5, 5, 247.5, True)],
            [(0, 100, 4, 110.0, False), (2, 255, 6, 880.0, True)],                                  # the held key's note-off; the last frame
            [],
            [(2, 0, 6, 880.0, False), (0, 128, 7, 165.0, True)]]


def test_detuned_player_equals_the_host_composition(ctx, oracle):
    """3 players, 6 buffers of 256 frames, main_delay 300 so that the echoes return inside the run; mode steps through 0, 1, 2, 3
    between buffers (and on): wide and narrow warble reach the voice with the next key, the echo bit at once"""
    from zang_amd.detuned import DetunedPlayer
    player = DetunedPlayer(ctx, N, sample_rate=dc.SR, first_seed=dc.FIRST_SEED, main_delay=MAIN_DELAY, patch=dc.gpu_patch(dc.TEST_PATCH))
    main = dr.MainModule(oracle, N, dc.SR, dc.FIRST_SEED, MAIN_DELAY, dc.TEST_PATCH)
    loudest, differ = 0.0, False
    for b, ev in enumerate(_pushes()):
        player.mode = main.mode = b & 3
        for e in ev:
            player.push(*e)
            main.push(*e)
        gl, gr = (np.ascontiguousarray(x.cpu().numpy()) for x in player.paint(F))
        wl, wr = main.paint(F)
        util.assert_bitexact(gl, wl, f"buffer {b} left")
        util.assert_bitexact(gr, wr, f"buffer {b} right")
        loudest = max(loudest, float(np.abs(wl).max()))
        differ = differ or not dc.same_bits(wl, wr)                  # the echoes have come back: left and right part
    assert loudest > 0.05 and differ and player.overflows() == 0
    assert ctx.last_form()[-1].startswith("k_stereo_echoes"), ctx.last_form()
    util.assert_bitexact(dr.struct_state(player.voices.state()), dr.state_words(main.voices), "state")
    player.close()
