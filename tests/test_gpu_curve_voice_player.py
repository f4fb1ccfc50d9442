"""GPU: CurvePlayer (zang_amd/sfx.py) -- N of examples/example_curve.zig's MainModule played live from pushed impulses -- against
MainModule composed on the host (tests/curve_player_reference.py: ImpulseQueue -> PolyphonyDispatcher -> Trigger from
zang_amd/notes.py, CurvePlayer.paint as oracle calls per sub-span).  A kit whose curves last about 700 frames under buffers of
256: every note crosses at least two buffer edges in the voices' carried state.  Everything on bits."""
import numpy as np
import pytest

from tests import curve_player_cases as cc
from tests import curve_player_reference as cr
from tests import util

pytestmark = pytest.mark.gpu
F, B = 256, 6


def _pushes(n_players):
    """per buffer (player, frame, note_id, effect, rel_freq) in push order: one at frame 0 and one at the last frame, two on ONE
    frame, two inside one buffer, the kit's count as an effect; the LAST player is never pushed to"""
    rng = np.random.default_rng(20261021)
    busy = n_players - 1
    out, nid = [], 1
    for b in range(B):
        ev = []

        def add(j, f, eff):
            nonlocal nid
            ev.append((j, f, nid, eff, float(np.float32(rng.uniform(0.5, 2.0)))))
            nid += 1
        if b == 0:
            add(0, 0, 0); add(0, F - 1, 1)                           # frame 0 and the last frame, both for player 0
        if b == 1:
            add(1, 40, 1); add(1, 40, 0)                             # two on one frame
        if b == 3:
            add(0, 30, 1); add(0, 200, 2)                            # two inside one buffer, the second with the kit's count
        if b in (2, 4):
            for j in range(1, busy):
                for f in sorted(rng.integers(0, F, int(rng.integers(0, 3))).tolist()):
                    add(j, f, int(rng.integers(0, 2)))
        out.append(ev)
    return out


@pytest.mark.parametrize("n_players,polyphony", [(5, 1), (3, 3)])
def test_curve_player_equals_the_host_composition(ctx, oracle, n_players, polyphony):
    """sync=True: the players' rows (polyphony > 1: zh_mixdown_groups over each player's voices, in voice order) and the
    frequency image per voice, six buffers, then the ten state words of every voice"""
    from zang_amd.sfx import CurvePlayer, SfxKit
    N, P = n_players, polyphony
    kit = SfxKit(ctx, cc.long_kit_effects())
    player = CurvePlayer(ctx, N, kit, polyphony=P, sample_rate=cc.SR, sync=True)
    main = cr.MainModule(oracle, cr.Kit(cc.long_kit_effects()), N, P, cc.SR)
    loudest, sounding, overlap = 0.0, [], False
    for b, ev in enumerate(_pushes(N)):
        for e in ev:
            player.push(*e)
            main.push(*e)
        got, got_sync = (x.cpu().numpy() for x in player.paint(F))
        rows, sync = main.paint(F)
        want = np.zeros((N, F), np.float32)
        for j in range(N):
            for i in range(P):
                want[j] = want[j] + rows[j * P + i]
        util.assert_bitexact(np.ascontiguousarray(got), want if P > 1 else rows, f"N={N} P={P} buffer {b}")
        util.assert_bitexact(np.ascontiguousarray(got_sync), sync, f"N={N} P={P} buffer {b} frequency image")
        loudest = max(loudest, float(np.abs(want).max()))
        sounding.append(bool(rows[0].any()))
        overlap = overlap or bool(((rows[0] != 0) & (rows[1] != 0)).any())
        assert not rows[(N - 1) * P:].any() and not sync[(N - 1) * P:].any()      # the player without a push stays silent
    # the note of buffer 0's frame 0 (P = 1: of its last frame) still sounds two buffers on: it crossed two buffer edges
    assert sounding[:3] == [True, True, True] and loudest > 0.5 and (P == 1 or overlap)
    assert player.overflows() == 0
    util.assert_bitexact(cr.struct_state(player.voices.state()), cr.state_words([v for row in main.voices for v in row]), "state")
    player.close(); kit.close()


def test_curve_player_without_sync_paints_one_image(ctx, oracle):
    """sync=False: paint() returns the players' rows alone and no frequency image exists"""
    from zang_amd.sfx import CurvePlayer, SfxKit
    kit = SfxKit(ctx, cc.long_kit_effects())
    player = CurvePlayer(ctx, 2, kit, sample_rate=cc.SR)
    main = cr.MainModule(oracle, cr.Kit(cc.long_kit_effects()), 2, 1, cc.SR)
    for b in range(2):
        if b == 0:
            player.push(0, 5, 1, 0, 1.5); main.push(0, 5, 1, 0, 1.5)
        got = player.paint(F)
        util.assert_bitexact(np.ascontiguousarray(got.cpu().numpy()), main.paint(F)[0], f"buffer {b}")
    assert player._sync is None and ctx.last_form()[-1] == "k_curve_player_spans", ctx.last_form()
    player.close(); kit.close()
