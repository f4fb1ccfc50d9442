"""GPU: VibratoPlayer and PortaPlayer (zang_amd/lead.py) -- N of the MainModules of examples/example_vibrato.zig and
examples/example_portamento.zig played live -- against the MainModule composed on the host (tests/lead_reference.py: ImpulseQueue ->
Trigger from zang_amd/notes.py, Instrument.paint as oracle calls per sub-span).  Everything on bits; 3 players x 4 buffers of 256."""
import numpy as np
import pytest

from tests import lead_cases as lc
from tests import lead_reference as lr
from tests import util

pytestmark = pytest.mark.gpu
F, N = 256, 3
KEY_FREQS = (110.0 * 2.0 ** (np.arange(64) / 12.0)).astype(np.float32)


def _compare(kind, player, main, b):
    ga, gs = (np.ascontiguousarray(x.cpu().numpy()) for x in player.paint(F))
    wa, ws = main.paint(F)
    util.assert_bitexact(ga, wa, f"buffer {b} audio")
    util.assert_bitexact(gs, ws, f"buffer {b} sync")
    return wa, ws


def test_vibrato_player_equals_the_host_composition(ctx, oracle):
    """per buffer (player, frame, note_id, freq, note_on) in push order, as keyEvent pushes them (a note-off only for the held key):
    two at one frame, a note-off, a new key while one is held; player 2 is pushed to once, on the last frame of a buffer"""
    from zang_amd.lead import VibratoPlayer
    kind = lc.VIBRATO
    pushes = [[(0, 0, 1, 220.0, True), (1, 17, 2, 330.0, True)],
              [(0, 40, 3, 440.0, True), (0, 40, 4, 110.0, True), (1, 200, 2, 330.0, False)],
              [(1, 5, 5, 247.5, True), (2, 255, 6, 880.0, True)],
              [(0, 100, 4, 110.0, False), (2, 0, 6, 880.0, False), (0, 128, 7, 165.0, True)]]
    player = VibratoPlayer(ctx, N, sample_rate=lc.SR, patch=kind.gpu_patch(kind.test_patch))
    main = lr.MainModule(oracle, kind.voice, kind.paint, N, lc.SR, kind.test_patch)
    loudest = 0.0
    for b, ev in enumerate(pushes):
        for e in ev:
            player.push(*e)
            main.push(*e)
        wa, ws = _compare(kind, player, main, b)
        loudest = max(loudest, float(np.abs(wa).max()))
    assert loudest > 0.5 and player.overflows() == 0
    assert ctx.last_form()[-1] == "k_lead_spans", ctx.last_form()
    util.assert_bitexact(lr.struct_state(kind.voice, player.voices.state()), lr.state_words(main.voices), "state")
    player.close()


# per buffer (player, key_index, down, frame)
KEY_SCRIPT = [[(0, 10, True, 0), (0, 20, True, 100), (0, 5, True, 150), (1, 63, True, 17)],       # a higher key glides; a lower one: no push
              [(0, 20, False, 40), (0, 10, True, 41), (1, 63, False, 200), (2, 0, True, 255)],    # highest released: on at key 10; a repeat; the last key up
              [(0, 10, False, 5), (0, 5, False, 90), (1, 30, True, 10)],                          # on at key 5, then off; player 1 restarts
              [(2, 0, False, 0), (0, 7, True, 128), (2, 1, True, 128), (2, 2, True, 128)]]        # two at one frame


def test_porta_player_equals_the_host_composition_under_the_key_rule(ctx, oracle):
    """PortaPlayer.key against the reference MainModule fed by an independent restatement of keyEvent (lr.PortaKeys: fresh ids on
    every push, a bare Trigger): glides between held keys, no envelope restart while a key is held, one at release"""
    from zang_amd.lead import PortaPlayer
    kind = lc.PORTA
    player = PortaPlayer(ctx, N, KEY_FREQS, sample_rate=lc.SR, patch=kind.gpu_patch(kind.test_patch))
    main = lr.MainModule(oracle, kind.voice, kind.paint, N, lc.SR, kind.test_patch)
    keys = [lr.PortaKeys(KEY_FREQS) for _ in range(N)]
    loudest, pushed, glided = 0.0, 0, False
    for b, ev in enumerate(KEY_SCRIPT):
        for p, k, down, frame in ev:
            got = player.key(p, k, down, frame)
            want = keys[p].key_event(k, down)
            assert (got is None) == (want is None) and (got is None or got[1:] == (float(want[1]), want[2])), (b, p, k, got, want)
            if want is not None:
                main.push(p, frame, *want)
                pushed += 1
        wa, ws = _compare(kind, player, main, b)
        loudest = max(loudest, float(np.abs(wa).max()))
        glided = glided or bool(((ws[0] > KEY_FREQS[10]) & (ws[0] < KEY_FREQS[20])).any())
    assert loudest > 0.3 and glided and pushed == 13 and player.overflows() == 0
    util.assert_bitexact(lr.struct_state(kind.voice, player.voices.state()), lr.state_words(main.voices), "state")
    assert [k.keys_held for k in player.keys] == [k.keys_held for k in keys] == [1 << 7, 1 << 30, (1 << 1) | (1 << 2)]
    player.close()
