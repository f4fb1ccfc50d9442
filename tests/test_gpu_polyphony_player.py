"""GPU: PolyphonyPlayer (zang_amd/polyphony.py) -- N x examples/example_polyphony.zig MainModule -- over six buffers of scripted key
events with the space bar pressed between them, end to end: the audio equals the model's (tests/polyphony_reference.py: the outer
Trigger and every key's own queue and Trigger in Python, the samples from the oracle's NiceInstrument and Decimator) on bits after
every buffer; and one buffer's launches recorded into a graph replay to the bits of the direct calls."""
import pytest

from tests import hostile_cases as hc
from tests import polyphony_cases as pc
from tests import polyphony_reference as pr

pytestmark = pytest.mark.gpu
CASE = pc.CASES[0]                                                     # 41 keys
F = pc.OUT_LEN


def _spaces(b, p):
    """space-bar presses of player p before buffer b: player 0 stays in mode 0 for two buffers, then walks 1, 2, ...; player 1 goes
    to mode 6 at once and on to 0 and 1; player 2 to mode 1 and stays -- modes 0, 1 and 6 all play, and differ between players"""
    return {0: [0, 0, 1, 1, 1, 1], 1: [6, 0, 0, 1, 0, 1], 2: [1, 0, 0, 0, 0, 0]}[p][b]


def _inner(rec, b, N):
    K = CASE.n_keys
    return [rec.inner[b][p * K:(p + 1) * K] for p in range(N)]


@pytest.mark.parametrize("N", [1, 3])
def test_the_player_equals_the_model_after_every_buffer(ctx, oracle, N):
    from zang_amd import polyphony
    rec = pc.run(CASE)
    player = polyphony.PolyphonyPlayer(ctx, N, CASE.key_freqs())
    buses = [pr.Bus(oracle, CASE.n_keys) for _ in range(N)]
    models = [pr.MainModule(CASE.key_freqs()) for _ in range(N)]       # for the space bar alone: the notes are rec's
    loud, seen = 0.0, set()
    for b in range(pc.BUFFERS):
        for p in range(N):
            for _ in range(_spaces(b, p)):
                assert player.space(p) == models[p].space()
            for (key, down, frame), pushed in zip(pc.script(CASE, p)[b], rec.pushed[b][p]):
                assert player.key(p, key, down, frame) == pushed[1:]                 # keyEvent: a fresh id and the whole mask
        audio = player.paint(F)
        ctx.sync()
        assert ctx.last_form() == ["k_mix_groups_decimated"], ctx.last_form()       # the last of the four calls
        modes = [m.dec_mode for m in models]
        seen.update(modes)
        ref = pr.render(oracle, buses, _inner(rec, b, N), modes, F)
        got = audio.cpu().numpy()
        assert got.shape == (N, F)
        assert hc.same_f32(got, ref), (f"buffer {b}", modes, hc.first_difference(got, ref))
        dec = player.dec.state()
        assert hc.same_f32(dec["dval"], [x.dec.dval for x in buses]) and hc.same_f32(dec["dcount"], [x.dec.dcount for x in buses]), f"buffer {b}"
        loud = max(loud, float(abs(ref).max()))
    assert loud > 0.1 and player.overflows() == 0
    assert seen >= ({0, 1, 6} if N == 3 else {0, 1})
    player.close()


def test_a_captured_buffer_replays_to_the_direct_launches(ctx):
    """the launches of one paint that a graph can hold -- the fan-out's schedule, the span paint of all the voices and the
    decimated group mix; the live bank's own schedule copies the pushed records from the host and is refused while a capture
    records, so it runs in front of the graph -- recorded (on a context of a side stream: capture needs a non-default one) and
    replayed ONCE: the replay leaves the audio, the table and every state the direct launches of the other player leave."""
    import torch
    import zang_amd
    from zang_amd import polyphony
    N = 3
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        direct, captured = (polyphony.PolyphonyPlayer(c2, N, CASE.key_freqs()) for _ in range(2))

        def keys(pl, b):
            for p in range(N):
                for key, down, frame in pc.script(CASE, p)[b]:
                    pl.key(p, key, down, frame)
        for pl in (direct, captured):
            for p, presses in enumerate((0, 6, 1)):                    # bypass, 1000 Hz and 6000 Hz
                for _ in range(presses):
                    pl.space(p)
            keys(pl, 0)
        first = [pl.paint(F).clone() for pl in (direct, captured)]     # buffer 0, both directly: the images and the modes exist
        keys(direct, 1); keys(captured, 1)
        want = direct.paint(F)
        captured.bank.schedule(F, polyphony.OUTER_SPANS)
        c2.sync()
        graph = c2.capture(lambda: captured.enqueue(F))
        assert [k for k, _ in graph.kernels()] == ["k_keyfan_schedule", "k_nice_spans", "k_mix_groups_decimated"], graph.kernels()
        graph.launch()
        c2.sync()
        got = captured._audio[:, :F]
        assert torch.equal(first[0].view(torch.int32), first[1].view(torch.int32))
        assert torch.equal(want.view(torch.int32), got.view(torch.int32)) and float(want.abs().max()) > 0.01
        assert not torch.equal(want[1], first[0][1])                   # (a buffer of its own, not the first one again)
        for a, b in ((direct.dec, captured.dec), (direct.stage, captured.stage), (direct.voices, captured.voices)):
            assert a.state().tobytes() == b.state().tobytes()
        assert pr.same_table(captured.stage.download(captured.max_spans), direct.stage.download(direct.max_spans)) is None
        graph.close()
        direct.close(); captured.close()
        c2.close()
