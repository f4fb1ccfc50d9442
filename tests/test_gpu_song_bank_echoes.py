"""GPU: SongBank(..., echoes=(main_delay, feedback_volume, cutoff)) -- N songs mixed per song, put through StereoEchoes on the
output bus (examples/example_delay.zig:69-79: StereoEchoes(15000), feedback 0.6, cutoff 0.1) and converted to interleaved stereo
s16 -- against an oracle render of each song: tests.test_song._oracle_song_render's loop with the oracle's StereoEchoes composition
between the f32 buffer and two zo_mixdown_s16lsb calls.  Payloads are compared byte for byte.  The six variants and the 2 s
(93 x 1,024 + 768 frames) are those of tests/test_gpu_song_bank.py."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_song_bank import _buffers, _songs
from tests.test_song import F, SR

pytestmark = pytest.mark.gpu
ECHOES = (15000, 0.6, 0.1)


def _oracle_song_render_echoes(oracle, notes, instruments, nbuf, last_frames, echoes):
    """_oracle_song_render (tests/test_song.py) with the bus effect: the instruments paint into a zeroed temp, StereoEchoes paints
    the zeroed outputs from it (example_delay.zig:53-79), mixDown converts each output into its channel (write_wav.zig:71-78)."""
    from zang_amd import song, zang
    L = oracle.lib()
    MAIN, fb, cutoff = echoes
    HALF = MAIN // 2
    sched = song.SongScheduler(notes, instruments)
    mods = []
    for inst in instruments:
        subs = []
        for _ in range(inst.polyphony):
            if inst.kind == "pmosc":
                m = oracle.PMOscInstrument(); L.zo_pmosc_init(C.byref(m), inst.init_arg)
            else:
                m = oracle.NiceInstrument(); L.zo_nice_init(C.byref(m), inst.init_arg)
            subs.append(m)
        mods.append(subs)
    r0, r1, re = np.zeros(HALF, np.float32), np.zeros(HALF, np.float32), np.zeros(MAIN, np.float32)
    d0 = oracle.Delay(); L.zo_delay_init(C.byref(d0), oracle.fptr(r0), HALF)
    d1 = oracle.Delay(); L.zo_delay_init(C.byref(d1), oracle.fptr(r1), HALF)
    de = oracle.Delay(); L.zo_delay_init(C.byref(de), oracle.fptr(re), MAIN)
    fl = oracle.Filter(); L.zo_filter_init(C.byref(fl))
    t0, t1, t2 = (np.zeros(F, np.float32) for _ in range(3))
    e0, e1, e2, e3 = (np.zeros(F, np.float32) for _ in range(4))
    payload = []
    for b in range(nbuf):
        n = last_frames if b == nbuf - 1 else F
        dry = np.zeros(F, np.float32)                                   # example_delay.zig:53
        outL, outR = np.zeros(F, np.float32), np.zeros(F, np.float32)   # write_wav.zig:63-64
        tables = sched.buffer(zang.Span(0, n))
        for inst, subs, per_voice in zip(instruments, mods, tables):
            for m, spans in zip(subs, per_voice):
                for (s, e, f, on, nic) in spans:                         # example_song.zig:336-347
                    if inst.kind == "pmosc":
                        L.zo_pmosc_paint(C.byref(m), s, e, oracle.fptr(dry), oracle.fptr(t0), oracle.fptr(t1), oracle.fptr(t2), int(nic), SR, f, int(on))
                    else:
                        L.zo_nice_paint(C.byref(m), s, e, oracle.fptr(dry), oracle.fptr(t0), oracle.fptr(t1), int(nic), SR, f, int(on))
        # StereoEchoes.paint, examples/modules.zig:494-523
        L.zo_add_into(0, n, oracle.fptr(outL), oracle.fptr(dry)); L.zo_add_into(0, n, oracle.fptr(outR), oracle.fptr(dry))
        L.zo_zero(0, n, oracle.fptr(e0)); L.zo_simple_delay_paint(C.byref(d0), 0, n, oracle.fptr(e0), oracle.fptr(dry))
        L.zo_zero(0, n, oracle.fptr(e1))
        L.zo_filtered_echoes_paint(C.byref(de), C.byref(fl), 0, n, oracle.fptr(e1), oracle.fptr(e2), oracle.fptr(e3), oracle.fptr(e0), fb, cutoff)
        L.zo_add_into(0, n, oracle.fptr(outL), oracle.fptr(e1))
        L.zo_simple_delay_paint(C.byref(d1), 0, n, oracle.fptr(outR), oracle.fptr(e1))
        dst = np.zeros(4 * n, np.uint8)
        L.zo_mixdown_s16lsb(dst.ctypes.data_as(C.POINTER(C.c_uint8)), oracle.fptr(outL), n, 2, 0, 0.25)   # write_wav.zig:71-78
        L.zo_mixdown_s16lsb(dst.ctypes.data_as(C.POINTER(C.c_uint8)), oracle.fptr(outR), n, 2, 1, 0.25)
        payload.append(dst.tobytes())
    return b"".join(payload)


@pytest.fixture(scope="module")
def references(ctx, oracle):
    """per variant: the oracle's 2 s stereo payload (a short last buffer: 96,000 = 93 x 1,024 + 768)"""
    from zang_amd import song
    _, six = _songs(ctx, 6)
    total, nbuf, last = _buffers(2.0)
    assert last == 768
    return [_oracle_song_render_echoes(oracle, notes, song.EXAMPLE_SONG_INSTRUMENTS, nbuf, last, ECHOES) for notes in six]


@pytest.fixture(scope="module")
def bank_of_six(ctx):
    """render(2.0) of the six variants with the default batch: what the other renders are compared with"""
    from zang_amd import songbank
    songs, _ = _songs(ctx, 6)
    bank = songbank.SongBank(ctx, songs, echoes=ECHOES)
    got = bank.render(2.0)
    assert bank.overflows() == 0
    bank.close()
    return got


def test_bank_of_six_with_echoes_equals_the_oracle(references, bank_of_six):
    got = bank_of_six
    assert len(got) == 6 and all(len(g) == 96000 * 4 for g in got)
    for i in range(6):
        assert got[i] == references[i], ("oracle", i)
    assert len(set(got)) == 6 and got[4] == bytes(96000 * 4)            # the song with no events stays silent


def test_echoes_recirculate_after_the_last_release_tail(bank_of_six):
    """The variant with the time scale 0.125 has its last note-off at 0.164 s; its payload is not silent in the last half second
    (frames 72,000 on: more than a second and four main delays later), on either channel, and the channels differ (the right one is
    the left one's echoes half a delay later)."""
    wet = np.frombuffer(bank_of_six[3], "<i2").reshape(-1, 2)
    tail = wet[72000:].astype(np.int32)
    assert np.abs(tail[:, 0]).max() > 0 and np.abs(tail[:, 1]).max() > 0
    assert not np.array_equal(tail[:, 0], tail[:, 1])


def test_split_render_with_echoes_equals_the_whole(ctx, bank_of_six):
    """render(1.0) twice: the cut (48,000 = 46 x 1,024 + 896) falls inside a buffer, so the second call goes back to the state before
    that buffer -- the echoes' rings, indices and filter included."""
    from zang_amd import songbank
    songs, _ = _songs(ctx, 6)
    bank = songbank.SongBank(ctx, songs, echoes=ECHOES)
    halves = [a + b for a, b in zip(bank.render(1.0), bank.render(1.0, batch=3))]
    assert halves == bank_of_six
    assert bank.overflows() == 0
    bank.close()


def test_batch_size_does_not_change_the_stereo_payload(ctx, bank_of_six):
    """batch = 1 (a paint of the echoes per buffer, as the reference does) against the default batch of 8 (one paint per eight)"""
    from zang_amd import songbank
    songs, _ = _songs(ctx, 6)
    bank = songbank.SongBank(ctx, songs, echoes=ECHOES)
    assert bank.render(2.0, batch=1) == bank_of_six
    bank.close()
