"""GPU: LaserPlayer (zang_amd/sfx.py) -- N of examples/example_laser.zig's MainModule played live from pushed impulses -- against
MainModule composed on the host (tests/laser_reference.py: ImpulseQueue -> PolyphonyDispatcher -> Trigger from zang_amd/notes.py,
LaserPlayer.paint as oracle calls per sub-span).  Everything on bits."""
import numpy as np
import pytest

from tests import laser_cases as lc
from tests import laser_reference as lr
from tests import util

pytestmark = pytest.mark.gpu
F, B = 256, 3


def _pushes(n_players):
    """per buffer (player, frame, note_id, effect, freq_mul, carrier_mul, modulator_mul, modulator_rad) in push order: two
    impulses for one player in one buffer, one at frame 0 and one at the last frame, one with frame >= the buffer's length
    (accepted, never painted), the kit's count as an effect; the LAST player is never pushed to"""
    rng = np.random.default_rng(20261019)
    busy = max(n_players - 1, 1)
    out, nid = [], 1
    for b in range(B):
        ev = []

        def add(j, f, eff):
            nonlocal nid
            ev.append((j, f, nid, eff, float(np.float32(rng.uniform(0.85, 1.15))), float(rng.choice([2.0, 4.0, 0.5, 1.0])),
                       float(rng.choice([0.5, 0.125, 9.0])), float(rng.choice([0.5, 1.0]))))
            nid += 1
        if b == 0:
            add(0, 0, 0); add(0, F - 1, 1)                           # frame 0 and the last frame, both for player 0
        if b == 1:
            add(0, 40, 4); add(0, 90, 1)                             # two inside one buffer
            add(0, F + 7, 3)                                         # past the buffer: accepted, never painted
        for j in range(1 if n_players > 1 else busy, busy):
            for f in sorted(rng.integers(0, F, int(rng.integers(0, 3))).tolist()):
                add(j, f, int(rng.integers(0, 6)))
        out.append(ev)
    return out


@pytest.mark.parametrize("n_players", [1, 3, 70])
def test_laser_player_equals_the_host_composition(ctx, oracle, n_players):
    from zang_amd.sfx import LaserPlayer, SfxKit
    kit = SfxKit(ctx, lc.kit_effects())
    player = LaserPlayer(ctx, n_players, kit, polyphony=1, sample_rate=lc.SR)
    main = lr.MainModule(oracle, lr.Kit(lc.kit_effects()), n_players, 1, lc.SR)
    loudest = 0.0
    for b, ev in enumerate(_pushes(n_players)):
        for e in ev:
            player.push(*e)
            main.push(*e)
        got = player.paint(F).cpu().numpy()
        want = main.paint(F)
        util.assert_bitexact(np.ascontiguousarray(got), want, f"N={n_players} buffer {b}")
        loudest = max(loudest, float(np.abs(want).max()))
        if n_players > 1:
            assert not want[n_players - 1].any()                     # the player without a push stays silent
    assert loudest > 0.05 and player.overflows() == 0
    assert ctx.last_form()[-1] == "k_laser_spans", ctx.last_form()
    util.assert_bitexact(lr.struct_state(player.voices.state()), lr.state_words([v for row in main.voices for v in row]), "state")
    player.close(); kit.close()


def test_laser_player_with_two_voices_mixes_them_down(ctx, oracle):
    """polyphony 2: a second impulse does not cut the first off; the player's row is zh_mixdown_groups over its two voices, in
    voice order"""
    from zang_amd.sfx import LaserPlayer, SfxKit
    N, P = 3, 2
    kit = SfxKit(ctx, lc.kit_effects())
    player = LaserPlayer(ctx, N, kit, polyphony=P, sample_rate=lc.SR)
    main = lr.MainModule(oracle, lr.Kit(lc.kit_effects()), N, P, lc.SR)
    overlap = False
    for b, ev in enumerate(_pushes(N)):
        for e in ev:
            player.push(*e)
            main.push(*e)
        got = player.paint(F).cpu().numpy()
        rows = main.paint(F)
        want = np.zeros((N, F), np.float32)
        for j in range(N):
            for i in range(P):
                want[j] = want[j] + rows[j * P + i]
        util.assert_bitexact(np.ascontiguousarray(got), want, f"buffer {b}")
        overlap = overlap or bool(((rows[0] != 0) & (rows[1] != 0)).any())
    assert overlap and player.overflows() == 0
    player.close(); kit.close()
