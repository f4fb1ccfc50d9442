"""GPU: MousePlayer (zang_amd/mouse.py) -- three live voice banks and ONE controlled phase-modulation paint a buffer, no
synchronisation -- against tests/mouse_reference.py's MainModule, the line-by-line restatement of examples/example_mouse.zig, per
player: the audio on bits after every one of 4 buffers of 128 frames of scripted events, for 3 and 70 players.  The events: mouse
moves mid-buffer, keys pressed, held and released, a release of a key that is not the held one, and `space` between buffers."""
import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import mouse_cases as mc
from tests import mouse_reference as mr

pytestmark = pytest.mark.gpu
f32 = np.float32
FRAMES, BUFFERS = 128, 4
REL_FREQS = [f32(2.0 ** (k / 12.0)) for k in range(-12, 13)]


def script(player):
    """one player's events -> [(buffer, frame, kind, ...)] sorted: ("m", x, y), ("k", key, down), and ("s",) before a buffer's
    first frame.  Player 1 plays nothing at all; player 0 holds a key across every edge, moves the mouse mid-buffer and releases a
    key that is not the held one; player 2 toggles the mode twice between two buffers (no change)."""
    if player == 1:
        return []
    if player == 0:
        return [(0, 0, "m", 0.25, 0.5), (0, 5, "k", 3, True), (0, 70, "m", 0.75, 0.125), (1, 0, "s"), (1, 40, "k", 5, False),
                (1, 41, "m", 0.5, 1.0), (2, 0, "s"), (2, 127, "k", 4, True), (3, 60, "k", 4, False), (3, 60, "m", 0.0, 0.0)]
    if player == 2:
        return [(0, 10, "k", 1, True), (0, 10, "m", 1.0, 1.0), (1, 0, "s"), (1, 0, "s"), (2, 64, "k", 1, False)]
    rng = np.random.default_rng(8800 + player)
    ev = []
    for b in range(BUFFERS):
        if b and rng.random() < 0.5:
            ev.append((b, 0, "s"))
        for frame in np.sort(rng.choice(FRAMES, int(rng.integers(0, 5)), replace=False)).tolist():
            if rng.random() < 0.5:
                ev.append((b, frame, "m", float(f32(rng.random())), float(f32(rng.random()))))
            else:
                ev.append((b, frame, "k", int(rng.integers(0, 4)), bool(rng.random() < 0.6)))
    return ev


@pytest.mark.parametrize("N", [3, 70])
@pytest.mark.parametrize("exact_temps", [True, False], ids=["exact_temps", "no_temp"])
def test_the_player_equals_main_module(ctx, oracle, N, exact_temps):
    """4 kHz, a4 = 110 and the tests' patch: the glides and the envelope's stages end inside the test.  Without exact_temps the
    model zeroes its stale temp before every buffer."""
    from zang_amd import modules as mod, mouse
    patch = mod.PMCtl.Patch(mc.PATCH.ctl_curve, mc.PATCH.ctl_glide, mc.PATCH.attack, mc.PATCH.decay, mc.PATCH.release, mc.PATCH.sustain_volume)
    player = mouse.MousePlayer(ctx, N, sample_rate=mc.SR, a4=110.0, patch=patch, exact_temps=exact_temps)
    models = [mr.MainModule(oracle, mc.SR, 110.0, mc.PATCH, zero_stale=not exact_temps) for _ in range(N)]
    scripts = [script(p) for p in range(N)]
    pushed = ignored = 0
    loud = 0.0
    for b in range(BUFFERS):
        for p in range(N):
            for ev in scripts[p]:
                if ev[0] != b:
                    continue
                if ev[2] == "s":
                    assert player.space(p) == (models[p].space() or models[p].keys.mode)
                elif ev[2] == "m":
                    player.mouse(p, ev[3], ev[4], ev[1]); models[p].mouse(ev[3], ev[4], ev[1])
                else:
                    rel = REL_FREQS[3 * ev[3] + 2]
                    got, want = player.key(p, ev[3], ev[4], rel, ev[1]), models[p].key(ev[3], ev[4], rel, ev[1])
                    assert (got is None) == (want is None) and (got is None or (got[1], got[2]) == want)
                    pushed += got is not None
                    ignored += got is None
        audio = player.paint(FRAMES)
        ctx.sync()
        assert ctx.last_form() == ["k_pmctl_controlled"], ctx.last_form()
        got = audio.cpu().numpy()
        ref = np.stack([m.paint(FRAMES) for m in models])
        assert hc.same_f32(got, ref), (f"buffer {b}", hc.first_difference(got, ref))
        loud = max(loud, float(np.abs(ref).max()))
    assert player.overflows() == 0 and pushed > N // 2 and ignored > 0 and loud > 0.01
    assert mr.same_words(mr.struct_state(player.voices.state()), mr.state_words([m.voice for m in models]))
    assert [k.mode for k in player.keys] == [m.keys.mode for m in models] and {k.mode for k in player.keys} == ({0, 1} if N > 3 else {0})
    player.close()
