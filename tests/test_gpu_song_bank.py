"""GPU: SongBank (zang_amd/songbank.py) -- N songs scheduled, painted, mixed per song in the reference's order and converted to
s16 in one set of launches per batch -- against the oracle's render of each song (tests.test_song._oracle_song_render) and
against SongRenderer(scheduler="device") on each song alone.  Payloads are compared byte for byte.

The songs are six variants of tests/golden/song_small.txt: pitches shifted, event times scaled and moved.  The golden song's
events all fall on whole frames (its rows are 1,800 to 14,400 frames long), where the f32 rounding of NoteTracker's clock
decides between frame n - 1 and n; every variant but the first moves its events half a frame off (scales that keep whole
frames, then + (k + 0.5) / 48000 s), where no rounding of a clock near 1 s (a few thousandths of a frame) can: a variant's
schedule then does not depend on how long the buffers are (checked on the host scheduler below).  The first stays as it is."""
import copy
import os
from unittest import mock

import numpy as np
import pytest

from tests.test_song import F, SR, _oracle_song_render

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (semitones, time scale, frames moved) -- None: a song with no events
VARIANTS = [(0, 1.0, 0.0), (3, 1.25, 0.5), (-5, 0.75, 10.5), (7, 0.125, 3.5), None, (-12, 2.0, 100.5)]
DENSE = 3


def _variant(v):
    from zang_amd import song
    notes = song.compile_song(open(os.path.join(ROOT, "tests", "golden", "song_small.txt")).read())
    if v is None:
        return [[] for _ in notes]
    semis, scale, moved = v
    for inst in notes:
        for e in inst:
            e.semis += semis
            e.t = float(np.float32(e.t) * np.float32(scale) + np.float32(moved / SR))
    return notes


def _songs(ctx, n):
    """n songs cycling through the variants (frequencies resolved on the device), and the six themselves"""
    from zang_amd import song
    six = [song.resolve_frequencies(_variant(v), ctx) for v in VARIANTS]
    return [six[i % len(six)] for i in range(n)], six


def _buffers(seconds):
    total = int(seconds * SR)
    nbuf = (total + F - 1) // F
    return total, nbuf, total - (nbuf - 1) * F


def _alone(ctx, notes, seconds):
    """SongRenderer(scheduler="device") on one song (its constructor compiles a text: hand it these events instead)"""
    from zang_amd import song
    with mock.patch.object(song, "compile_song", lambda text, instruments=song.EXAMPLE_SONG_INSTRUMENTS: copy.deepcopy(notes)):
        r = song.SongRenderer("", ctx, scheduler="device")
    out = r.render(seconds)
    assert all(b.overflows() == 0 for b in r.banks)
    return out


@pytest.fixture(scope="module")
def references(ctx, oracle):
    """per variant: the oracle's and the single-song renderer's 2 s payloads (a short last buffer: 96,000 = 93 x 1,024 + 768)"""
    from zang_amd import song
    _, six = _songs(ctx, 6)
    total, nbuf, last = _buffers(2.0)
    assert last == 768
    ref = [_oracle_song_render(oracle, notes, song.EXAMPLE_SONG_INSTRUMENTS, nbuf, last_frames=last) for notes in six]
    alone = [_alone(ctx, notes, 2.0) for notes in six]
    return ref, alone


def test_the_variants_are_distinct_one_is_empty_and_one_is_dense():
    from zang_amd import song, zang
    six = [_variant(v) for v in VARIANTS]
    keys = [tuple((round(e.t * SR, 2), e.semis, e.note_on) for inst in notes for e in inst) for notes in six]
    assert len(set(keys)) == 6 and keys[4] == ()
    for notes in six:                                               # (frequencies only have to be there for the host scheduler)
        for inst in notes:
            for e in inst:
                e.freq = 440.0
    sched = song.SongScheduler(six[DENSE])
    most = 0
    for _ in range(12):
        most = max(most, max(len(spans) for per_voice in sched.buffer(zang.Span(0, F)) for spans in per_voice))
    assert most >= 3, most


def test_bank_of_six_equals_the_oracle_and_the_single_song_renderer(ctx, references):
    from zang_amd import songbank
    ref, alone = references
    songs, _ = _songs(ctx, 6)
    bank = songbank.SongBank(ctx, songs)
    got = bank.render(2.0)
    assert len(got) == 6 and all(len(g) == 96000 * 2 for g in got)
    for i in range(6):
        assert got[i] == ref[i], ("oracle", i)
        assert got[i] == alone[i], ("SongRenderer", i)
    assert len(set(got)) == 6 and got[4] == bytes(96000 * 2)
    assert all(np.abs(np.frombuffer(g, "<i2").astype(np.int32)).max() > 1000 for i, g in enumerate(got) if i != 4)
    assert bank.overflows() == 0
    bank.close()


def test_from_texts_equals_the_single_song_renderer(ctx):
    from zang_amd import song, songbank
    text = open(os.path.join(ROOT, "tests", "golden", "song_small.txt")).read()
    bank = songbank.SongBank.from_texts(ctx, [text, text])
    got = bank.render(0.5, batch=5)
    want = song.SongRenderer(text, ctx, scheduler="device").render(0.5)
    assert got == [want, want] and bank.overflows() == 0
    bank.close()


@pytest.mark.parametrize("batch", [1, 8])
def test_bank_of_1024_equals_the_oracle_and_the_single_song_renderer(ctx, references, batch):
    from zang_amd import songbank
    ref, alone = references
    songs, _ = _songs(ctx, 1024)
    bank = songbank.SongBank(ctx, songs)
    got = bank.render(2.0, batch=batch)
    assert len(got) == 1024
    wrong = [i for i in range(1024) if got[i] != ref[i % 6] or got[i] != alone[i % 6]]
    assert not wrong, (len(wrong), wrong[:8])
    assert bank.overflows() == 0
    bank.close()


def test_state_carries_from_call_to_call(ctx):
    """Two renders of 1 s equal one of 2 s, and three of 0.7 s, 0.01 s and 1.29 s too.  Cut as write_wav cuts each call on its own
    (46 x 1,024 + 896 twice against 93 x 1,024 + 768) they could not: NoteTracker's clock is an f32 sum over buffers, and the
    PMOsc wraps its phase once per paint call, so the ORACLE's render of these songs differs between the two cuts from frame
    48,000 on (24,378 of 96,000 s16 samples of the second variant; the NiceInstruments are the same under both).  SongBank.render
    therefore keeps every buffer but the stream's last on one grid (its docstring): what is compared here is a call's short last
    buffer (896, 832 and 288 frames) against the same frames of the whole buffer; no event of any variant falls in one of them."""
    from zang_amd import songbank
    songs, _ = _songs(ctx, 12)
    one, two, three = (songbank.SongBank(ctx, songs) for _ in range(3))
    whole = one.render(2.0)
    halves = [a + b for a, b in zip(two.render(1.0), two.render(1.0, batch=3))]
    thirds = [a + b + c for a, b, c in zip(three.render(0.7), three.render(0.01), three.render(1.29, batch=5))]
    assert len(whole) == 12 and all(len(w) == 96000 * 2 for w in whole)
    assert halves == whole
    assert thirds == whole
    assert len(set(whole)) == 6 and one.overflows() == 0 and two.overflows() == 0 and three.overflows() == 0
    # and the stream goes on: a third second after the two equals the third second of three at once
    more = one.render(1.0)
    assert [a + b for a, b in zip(halves, two.render(1.0))] == [a + b for a, b in zip(whole, more)]
    for b in (one, two, three):
        b.close()


def test_two_calls_equal_two_calls_of_the_single_song_renderer_where_no_buffer_is_cut_short(ctx):
    """With calls that end on the buffer grid (1,024 x 40 frames each) nothing is rendered twice: the bank's second call equals
    SongRenderer's second call on each song."""
    from zang_amd import song, songbank
    songs, six = _songs(ctx, 6)
    bank = songbank.SongBank(ctx, songs)
    sec = 40 * F / SR
    got = [bank.render(sec), bank.render(sec)]
    for i, notes in enumerate(six):
        with mock.patch.object(song, "compile_song", lambda text, instruments=song.EXAMPLE_SONG_INSTRUMENTS: copy.deepcopy(notes)):
            r = song.SongRenderer("", ctx, scheduler="device")
        assert [got[0][i], got[1][i]] == [r.render(sec), r.render(sec)], i
    assert bank.overflows() == 0
    bank.close()
