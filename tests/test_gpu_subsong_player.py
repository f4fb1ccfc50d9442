"""GPU: SubsongPlayer (zang_amd/subsong.py) -- N x examples/example_subsong.zig MainModule -- over six buffers of scripted key
events, end to end: the mono image equals the model's (tests/subsong_reference.py: keyEvent, both Triggers, the NoteTracker and the
stage's arithmetic in Python, the samples from the oracle's TriSawOsc and Envelope) on bits; every buffer is exactly three
launches; a captured buffer replays to what the direct launches give."""
import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import subsong_cases as sc
from tests import subsong_reference as sr

pytestmark = pytest.mark.gpu
RATE = 4000.0                                      # the voice's own: the melody's notes lie inside the oscillator's 0 .. 500 Hz
F = sc.OUT_LEN


def key_script(p):
    """-> per buffer, player p's key events [(key, down, frame, melody)]: a press, a press of another key over it, a release of
    a key that is NOT down (ignored, :190), the release of the one that is, a press on a buffer's last frame, two presses in one
    buffer; neighbouring players play different melodies"""
    k0, k1, d, m = float(sc.key_freq(p)), float(sc.key_freq(p + 4)), (p * 5) % 23, p % 4
    return [[(k0, True, d, m)],
            [(k1, True, 60 + d, (m + 1) % 4), (k0, False, 100 + d, 0)],
            [(k1, False, 10 + d, 0), (k1, False, 50, 0)],
            [(k0, True, F - 1, sc.M_REF)],
            [(k0, True, 5, sc.M_DENSE), (k1, True, 200 - d, sc.M_REF)],
            []]


@pytest.fixture(scope="module")
def kit(ctx):
    from zang_amd import subsong
    k = subsong.MelodyKit(ctx, sc.KIT)
    yield k
    k.close()


@pytest.mark.parametrize("N", [1, 65])
def test_the_player_equals_the_model(ctx, oracle, kit, N):
    from zang_amd import subsong
    player = subsong.SubsongPlayer(ctx, N, kit, sample_rate=RATE, base_freq=sc.BASE_FREQ)
    model = [sr.Player(sc.KIT, sc.BASE_FREQ) for _ in range(N)]
    voices = [sr.InnerVoice(oracle) for _ in range(N)]
    loud, ignored = 0.0, 0
    for b in range(sc.BUFFERS):
        for p in range(N):
            for key, down, frame, melody in key_script(p)[b]:
                got, want = player.key_event(p, key, down, frame, melody), model[p].key_event(sr.f32(key), down, frame, melody)
                assert (got is None) == (want is None) and (got is None or got[1] == want[1])
                ignored += got is None
        audio = player.paint(F)
        ctx.sync()
        assert ctx.last_form() == ["k_saw_env_spans"], ctx.last_form()              # the last of paint()'s three calls
        inner = [model[p].schedule(F, RATE)[1] for p in range(N)]
        ref = sr.render(oracle, voices, inner, F, RATE)
        got = audio.cpu().numpy()
        assert hc.same_f32(got, ref), (f"buffer {b}", hc.first_difference(got, ref))
        assert sc.state_words(player.stage.state()) == [model[p].player.words() for p in range(N)], f"buffer {b}: the stage's state"
        loud = max(loud, float(np.abs(ref).max()))
    assert loud > 0.1 and ignored == 2 * N and player.overflows() == 0            # the release under another key, the second release
    player.close()


class _Recorder:
    """the library as the player's objects call it, with every zh_* call noted beside the kernels it launched (zh_last_form)"""

    def __init__(self, ctx):
        self._lib, self._ctx, self.calls = ctx.lib, ctx, []

    def _forms(self):
        import ctypes as C
        buf = C.create_string_buffer(512)
        assert self._lib.zh_last_form(self._ctx.handle, buf, 512) == 0
        return [k for k in buf.value.decode().split(",") if k]

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("zh_") or name == "zh_last_form":
            return fn

        def call(*args):
            rc = fn(*args)
            self.calls.append((name, self._forms()))
            return rc
        return call


def test_a_buffer_is_three_launches(ctx, kit, monkeypatch):
    """SubsongPlayer.paint() itself, with the library its objects call replaced by a recorder: per buffer exactly three library
    calls, each of which launched exactly one kernel -- no zero, no copy, no synchronise beside them"""
    from zang_amd import subsong
    N = 65
    player = subsong.SubsongPlayer(ctx, N, kit, sample_rate=RATE, base_freq=sc.BASE_FREQ)
    player.paint(F)                                                   # the first call allocates the image
    rec = _Recorder(ctx)
    for o in (ctx, player.bank, player.stage, player.voices):
        monkeypatch.setattr(o, "lib", rec)
    for b in range(2):
        for p in range(N):
            for key, down, frame, melody in key_script(p)[b]:
                player.key_event(p, key, down, frame, melody)
        del rec.calls[:]
        audio = player.paint(F)
        calls = list(rec.calls)
        assert [n for n, _ in calls] == ["zh_voice_bank_schedule_live", "zh_subsong_schedule", "zh_saw_env_paint_spans"], calls
        assert [len(k) for _, k in calls] == [1, 1, 1] and "k_voice_bank_schedule" in calls[0][1][0] and \
            [k for _, k in calls[1:]] == [["k_subsong_schedule"], ["k_saw_env_spans"]], calls
        ctx.sync()
        assert float(audio.abs().max()) > 0.05
    monkeypatch.undo()
    player.close()


def test_a_captured_buffer_replays_to_the_direct_launches(ctx):
    """the stage's schedule and the span paint of one buffer recorded into a graph (on a context of a side stream: capture needs
    a non-default one): after both players' banks ran the same pushes, every replay leaves the table, the state and the image
    the direct launches leave.  While the capture records, reserve is refused."""
    import torch
    import zang_amd
    from zang_amd import abi, subsong, zang
    N = 65
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        kit2 = subsong.MelodyKit(c2, sc.KIT)
        players = [subsong.SubsongPlayer(c2, N, kit2, sample_rate=RATE, base_freq=sc.BASE_FREQ) for _ in range(2)]
        direct, captured = players
        imgs = [c2.image(F, N, fill=0.5) for _ in range(2)]
        refused = []

        def record():
            refused.append(c2.lib.zh_subsong_reserve(captured.stage.handle, 99))
            captured.stage.schedule(RATE, F, captured.max_spans, captured._outer)
            captured.voices.paint_spans(zang.Span(0, F), [imgs[1]], None, captured._params, captured._table, zero_first=True)
        graph = None
        for b in range(3):
            for pl in players:
                for p in range(N):
                    for key, down, frame, melody in key_script(p)[b]:
                        pl.key_event(p, key, down, frame, melody)
                pl.bank.schedule(F, subsong.OUTER_SPANS)
            direct.stage.schedule(RATE, F, direct.max_spans, direct._outer)
            direct.voices.paint_spans(zang.Span(0, F), [imgs[0]], None, direct._params, direct._table, zero_first=True)
            c2.sync()
            if graph is None:
                graph = c2.capture(record)
                assert refused == [abi.ZH_ERR_UNSUPPORTED]
                assert [k for k, _ in graph.kernels()] == ["k_subsong_schedule", "k_saw_env_spans"], graph.kernels()
            graph.launch()
            c2.sync()
            assert torch.equal(imgs[0].view(torch.int32), imgs[1].view(torch.int32)), f"buffer {b}"
            assert direct.stage.state().tobytes() == captured.stage.state().tobytes()
            assert sr.same_table(captured.stage.download(captured.max_spans), direct.stage.download(direct.max_spans)) is None
            assert float(imgs[0].abs().max()) > 0.05
        graph.close()
        for pl in players:
            pl.close()
        kit2.close(); c2.close()
