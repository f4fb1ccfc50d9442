"""GPU: TwoPlayer (zang_amd/two.py) -- two live voice banks, the merge stage and the Dual span paint, four launches a buffer and
no synchronisation -- against tests/two_reference.py's MainModule, the line-by-line restatement of examples/example_two.zig, per
player: the audio image and the frequency image on bits after every buffer of scripted key events, for 1, 3 and 65 players, in
buffers of 256 frames and the same events in buffers of 128 and 384."""
import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import two_reference as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
TOTAL = 1024                                       # 4 buffers of 256, 8 of 128; 384: 3 buffers, the events past 1024 never come
REL_FREQS = [f32(2.0 ** (k / 12.0)) for k in range(-12, 13)]


def script(player, total=TOTAL):
    """one player's key events in absolute frames, sorted: (frame, "k" or "n", key, down).  A few keys per source, so that presses
    land on a held key and releases on keys that are not the source's own; player 1 plays nothing at all"""
    if player == 1:
        return []
    rng = np.random.default_rng(4200 + player)
    ev = []
    for kind, n_keys in (("k", 4), ("n", 9)):
        for frame in np.sort(rng.choice(total, int(rng.integers(6, 14)), replace=False)).tolist():
            ev.append((frame, kind, int(rng.integers(0, n_keys)), bool(rng.random() < 0.55)))
    if player == 0:                                # both sources at frame 0, a tie inside a buffer, a press on the last frame
        ev += [(0, "k", 2, True), (0, "n", 8, True), (300, "k", 1, True), (300, "n", 0, True), (total - 1, "k", 3, True)]
    return sorted(ev, key=lambda e: (e[0], e[1]))


def _rel(key):
    return REL_FREQS[3 * key + 2]


@pytest.mark.parametrize("frames", [256, 128, 384])
@pytest.mark.parametrize("N,sample_rate,a4", [(1, 48000, 880.0), (3, 4000, 110.0), (65, 4000, 110.0)], ids=["1", "3", "65"])
def test_the_player_equals_main_module(ctx, oracle, N, sample_rate, a4, frames):
    """at 48 kHz the example's own constants; at 4 kHz and a4 = 110 the envelope's stages end inside the test"""
    from zang_amd import two
    player = two.TwoPlayer(ctx, N, sample_rate=sample_rate, a4=a4)
    models = [tr.MainModule(oracle, a4, sample_rate) for _ in range(N)]
    scripts = [script(p) for p in range(N)]
    buffers = -(-TOTAL // frames)
    pushed = 0
    for b in range(buffers):
        lo, hi = b * frames, (b + 1) * frames
        for p in range(N):
            for frame, kind, key, down in scripts[p]:
                if lo <= frame < hi:
                    if kind == "k":
                        ev = player.note_key(p, key, down, _rel(key), frame - lo)
                        models[p].key_event(key, down, frame - lo, rel_freq=_rel(key))
                    else:
                        ev = player.number_key(p, key, down, frame - lo)
                        models[p].key_event(key, down, frame - lo, number=key)
                    pushed += ev is not None
        audio, sync = player.paint(frames)
        ctx.sync()
        assert ctx.last_form() == ["k_dual_spans"], ctx.last_form()
        got_a, got_s = audio.cpu().numpy(), sync.cpu().numpy()
        ref_a, ref_s = np.zeros((N, frames), f32), np.zeros((N, frames), f32)
        temps = [np.zeros(frames, f32) for _ in range(2)]
        for p in range(N):
            models[p].paint(frames, (ref_a[p], ref_s[p]), temps)
        assert hc.same_f32(got_a, ref_a), (f"buffer {b}: audio", hc.first_difference(got_a, ref_a))
        assert hc.same_f32(got_s, ref_s), (f"buffer {b}: sync", hc.first_difference(got_s, ref_s))
        table = player.stage.download(two.MAX_SPANS)
        assert [int(c) for c in table["count"]] == [len(m.rows) for m in models], f"buffer {b}: rows"
        assert all(m.rows[0][0] == 0 and m.rows[-1][1] == frames for m in models)          # both sources cover every buffer
    assert player.overflows() == 0 and pushed > 4 * (N - (N > 1))
    assert float(np.abs(ref_a).max()) > 0.01 and float(ref_s.min()) >= f32(a4) * f32(0.5)
    ids0 = [m.next_id0 for m in models]
    assert ids0 == [k._next0 for k in player.keys] and [m.next_id1 for m in models] == [k._next1 for k in player.keys]
    player.close()

