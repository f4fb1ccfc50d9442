"""GPU: ArpPlayer (zang_amd/arp.py) -- N x examples/example_arpeggiator.zig MainModule -- over six buffers of scripted key events,
end to end: audio and sync equal the model's (tests/arp_reference.py: both Triggers and the arpeggiator in Python, the samples from
the oracle) on bits, and equal what a host that runs the arpeggiator itself gets today -- ArpKeys' pushes through a LiveVoiceBank
for the outer sub-spans, then HardSquare.paint_spans fed the model's table."""
import numpy as np
import pytest

from tests import arp_cases as ac
from tests import arp_reference as ar
from tests import hostile_cases as hc
from tests import util

pytestmark = pytest.mark.gpu
CASES = [c for c in ac.CASES if c.name in ("nd100", "nd7")]


@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_player_equals_the_model_and_the_host_side_composition(ctx, oracle, case, N):
    from zang_amd import arp, modules as mod, zang
    from zang_amd.bank import LiveVoiceBank
    rec = ac.run(case)
    F = ac.OUT_LEN
    player = arp.ArpPlayer(ctx, N, case.key_freqs(), sample_rate=case.sample_rate, max_spans=case.max_spans)
    voices = [ar.HardSquareVoice(oracle) for _ in range(N)]
    # the host-side composition: its own keys, bank and voice
    keys = [arp.ArpKeys(case.n_keys) for _ in range(N)]
    bank = LiveVoiceBank(ctx, N, 1, arp.HELD_PARAMS, arp.HELD_PARAMS.fields["on"][1], 33 * N, rows=ac.OUTER_SPANS)
    host_voice = mod.HardSquare(N, ctx)
    loud = 0.0
    for b in range(ac.BUFFERS):
        for p in range(N):
            for (key, down, frame), pushed in zip(ac.script(case, p)[b], rec.pushed[b][p]):
                assert player.key(p, key, down, frame) == pushed[1:]                 # keyEvent: a fresh id and the whole mask
                note_id, held = keys[p].key(key, down)
                r = np.zeros(1, arp.HELD_PARAMS)
                r["held_lo"], r["held_hi"], r["on"] = held & 0xffffffff, held >> 32, 1
                bank.push(p, frame, note_id, r)
        audio, sync = player.paint(F)
        bank.schedule(F, ac.OUTER_SPANS)
        ctx.sync()
        ref, rsync = ar.render(oracle, voices, rec.inner[b][:N], F, case.sample_rate)
        got, gsync = audio.cpu().numpy(), sync.cpu().numpy()
        assert hc.same_f32(got, ref), (f"buffer {b} audio", hc.first_difference(got, ref))
        assert hc.same_f32(gsync, rsync), (f"buffer {b} sync", hc.first_difference(gsync, rsync))
        assert np.array_equal(player.voices.state()["osc"]["cnt"], np.array([v.cnt for v in voices], np.uint32)), f"buffer {b} state"
        # the outer sub-spans a host would run its arpeggiator over are the model's ...
        outer = bank.download(ac.OUTER_SPANS)
        for p in range(N):
            want = rec.outer[b][p]
            assert int(outer["count"][p]) == len(want)
            for k, (s, e, held, _) in enumerate(want):
                m = ac.mask_of(held)
                assert (int(outer["start"][k, p]), int(outer["end"][k, p]), int(outer["words"][0, k, p]), int(outer["words"][1, k, p])) == \
                    (s, e, m & 0xffffffff, m >> 32), (b, p, k)
        # ... and the voice fed the table that arpeggiator makes paints what the player painted
        tb, dropped = ar.table(rec.inner[b][:N], case.max_spans)
        assert dropped == 0
        table = host_voice.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], {"freq": (tb["freq"], None), "note_on": (None, tb["note_on"])})
        himg, hsync = ctx.image(F, N, fill=0.5), ctx.image(F, N, fill=0.5)
        host_voice.paint_spans(zang.Span(0, F), [himg, hsync], None, host_voice.Params(case.sample_rate), table, zero_first=True)
        ctx.sync()
        assert hc.same_f32(util.from_image(himg), got) and hc.same_f32(util.from_image(hsync), gsync), f"buffer {b}: the two paths differ"
        loud = max(loud, float(np.abs(ref).max()))
    assert loud > 0.1 and player.overflows() == 0
    player.close(); bank.close(); host_voice.close()


def test_overflows_sums_both_stages(ctx):
    """max_spans far too small: the stage drops rows and counts them, the player reports them"""
    from zang_amd import arp
    case = next(c for c in ac.CASES if c.name == "overflow")
    N = 65
    rec = ac.run(case)
    player = arp.ArpPlayer(ctx, N, case.key_freqs(), sample_rate=case.sample_rate, max_spans=case.max_spans)
    dropped = 0
    for b in range(2):
        for p in range(N):
            for key, down, frame in ac.script(case, p)[b]:
                player.key(p, key, down, frame)
        player.paint(ac.OUT_LEN)
        dropped += ar.table(rec.inner[b][:N], case.max_spans)[1]
    assert dropped > 0 and player.overflows() == dropped
    player.close()
