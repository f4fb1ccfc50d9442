"""CPU: the subsong tests' model (tests/subsong_reference.py) and case list (tests/subsong_cases.py) themselves: the model's consume
and walk agree with the oracle's (oracle/zs_interp.py, imported, not edited) where their semantics coincide, the reference melody
gives hand-derived rows, and every named case does what its name says."""
import numpy as np
import pytest

from oracle import zs_interp as zi
from tests import subsong_cases as sc
from tests import subsong_reference as sr

f32 = np.float32


@pytest.mark.parametrize("rate", [2000.0, 1024.0, 3001.0, 0.0, -2000.0, float("nan"), float("inf")])
def test_consume_is_the_oracles(rate):
    """a song whose ids are index + 1 (the oracle's convention), consumed over uneven sub-spans: frames, next and t"""
    song = [(f32(0.013 * i), i + 1, f32(100 + i), True) for i in range(60)]
    tr, st = sr.NoteTracker(song), {"next": 0, "t": f32(0)}
    for s, e in [(0, 256), (0, 77), (77, 78), (78, 256), (0, 256), (3, 250)]:
        r = rate if (s, e) != (0, 77) else 2000.0                    # one sane call among the hostile ones
        got = tr.consume(r, s, e)
        want = zi.note_tracker_consume(st, [t for t, *_ in song], r, s, e)
        assert [(fr, i) for fr, i, _ in got] == [(fr, i) for fr, i, _ in want]
        assert tr.next_song_event == st["next"] and sr.bits(tr.t) == sr.bits(st["t"])


def test_walk_is_the_oracles():
    rng = np.random.default_rng(7)
    trig, cur = sr.Trigger(), None
    for _ in range(200):
        frames = sorted(int(x) for x in rng.integers(0, 64, int(rng.integers(0, 6))))
        imps = [(fr, int(rng.integers(1, 4)), ("p", k)) for k, fr in enumerate(frames)]
        s = int(rng.integers(0, 20))
        e = s + int(rng.integers(1, 60))
        imps = [i for i in imps if s <= i[0]]                        # the oracle takes no impulse below the span's start
        want, cur = zi.trigger_spans(cur, imps, s, e)
        assert trig.spans(s, e, imps) == want
        assert (trig.note is None) == (cur is None) and (cur is None or trig.note == cur)


def test_hand_derived_rows_of_the_reference_melody():
    """sample rate 1024: a buffer of 256 frames is exactly 0.25 s, the clock's sums are exact, and event k at f32(0.1 k) s lands
    on frame trunc(f32(0.1 k) * 1024) of the song: 0, 102, 204, 307, 409, 512 -- f32(0.1 k) lies above 0.1 k for k = 1, 2, 3, 4 by
    far less than a frame's 1/1024 s, and 0.5 is exact, so the note-off is NOT below buffer 1's end_t 0.5 and opens buffer 2."""
    pl = sr.Player(sc.KIT, sc.BASE_FREQ)
    key = sc.BASE_FREQ
    pl.push(0, 1, key, True, sc.M_REF)
    want = [
        [(0, 102, 0, True, True), (102, 204, 1, True, True), (204, 256, 2, True, True)],
        [(0, 51, 2, True, False), (51, 153, 3, True, True), (153, 256, 4, True, True)],
        [(0, 256, 5, False, False)],                                  # the note-off has the last note-on's id: not a new note
        [(0, 256, 5, False, False)],
    ]
    for b, rows in enumerate(want):
        _, inner = pl.schedule(256, 1024.0)
        freqs = [(sc.REFERENCE_MELODY[k][2] * key) / sc.BASE_FREQ for _, _, k, _, _ in rows]     # :140, in f32
        assert inner == [(s, e, (f, on), nic) for (s, e, _, on, nic), f in zip(rows, freqs)], b
    assert pl.player.words()[:5] == [6, sr.bits(f32(1.0)), 0, 1, 5]
    # the melody whose note-off has its own id: the same rows, but the note-off IS a new note
    pl = sr.Player(sc.KIT, sc.BASE_FREQ)
    pl.push(0, 1, key, True, sc.M_OFF_NEW_ID)
    for b in range(3):
        _, inner = pl.schedule(256, 1024.0)
    assert [(s, e, on, nic) for s, e, (_, on), nic in inner] == [(0, 256, False, True)]


def test_the_uneven_cut_moves_the_clock_to_other_bits():
    """three calls of consume over 7 + 29 + 220 frames leave another f32 t than one call over 256"""
    cut, whole = sc.run(sc.case("uneven_outer_cut")), sc.run(sc.case("reference_melody_held"))
    assert [(s, e) for s, e, _, _ in cut.outer[1][0]] == [(0, 7), (7, 36), (36, 256)]
    assert [(s, e) for s, e, _, _ in whole.outer[1][0]] == [(0, 256)]
    assert cut.words[0][0][1] == whole.words[0][0][1] and cut.words[1][0][1] != whole.words[1][0][1]


def _stat(name, key):
    return sum(s[key] for s in sc.run(sc.case(name)).stats)


def test_every_named_case_does_what_its_name_says():
    n = max(sc.PLAYERS)
    assert _stat("reference_melody_held", "resets") == n
    held = sc.run(sc.case("reference_melody_held"))
    assert held.words[-1][0][0] == len(sc.REFERENCE_MELODY) and held.words[-1][0][6] == 0          # played to its end: the note-off is carried
    rel = sc.run(sc.case("release_mid_melody"))
    assert _stat("release_mid_melody", "resets") == n and rel.words[-1][0][0] == len(sc.REFERENCE_MELODY)
    assert any(not o[2][1] for o in rel.outer[1][0])                                              # an outer note-off ...
    assert any(on for _, _, (_, on), _ in rel.inner[2][0])                                        # ... under which the melody's notes go on
    assert _stat("repress_mid_melody", "resets") == 2 * n
    two = sc.run(sc.case("two_presses_one_buffer"))
    assert _stat("two_presses_one_buffer", "resets") == 3 * n and len(two.outer[0][0]) == 2     # buffer 2: two at ONE frame, the first has no frame
    kc = sc.run(sc.case("key_change_carried_note"))
    assert _stat("key_change_carried_note", "resets") == n
    a, b = kc.inner[1][0][:2]                              # the carried inner note, before and after the key's frequency changed
    assert a[1] == b[0] == 100 and not b[3] and sr.bits(a[2][0]) != sr.bits(b[2][0])
    assert any(e - s == 1 for s, e, _, _ in sc.run(sc.case("one_frame_outer")).outer[1][0])
    clamp = sc.run(sc.case("clamped_impulse"))
    assert all(st["clamped"] == 1 for st in clamp.stats)                                          # unclamped, rel is out_len (asserted in clamp_time too)
    assert [(s, e) for s, e, _, _ in clamp.outer[0][0]] == [(0, 2), (2, 7), (7, 256)]
    assert [(s, e, nic) for s, e, _, nic in clamp.inner[0][0]] == [(0, 2, True), (2, 6, False), (6, 7, True), (7, 256, False)]   # frame 6 = 2 + (5 - 1)
    assert all(w[0] == 2 and w[4] == 2 for w in clamp.words[0])                                   # the second event was taken, and it sounds
    assert _stat("last_frame_impulse", "clamped") == 0 and _stat("last_frame_impulse", "at_last") >= n
    last = sc.run(sc.case("last_frame_impulse"))
    assert last.inner[1][0][-1][:2] == (255, 256) and last.inner[1][0][-1][3]
    assert _stat("same_frame_events", "same_frame") >= 2 * n
    dense = sc.run(sc.case("more_than_32_events"))
    assert all(s["dropped"] > 0 for s in dense.stats)
    assert {len(x) for x in dense.inner[0]} == {32} and max(len(x) for x in dense.inner[1]) == 33   # 33: the carried note + 32 impulses, the most
    ids = sc.run(sc.case("note_off_ids"))
    assert [nic for _, _, (_, on), nic in ids.inner[3][0] if not on] == [False]                    # the shared id: no new note
    assert [nic for _, _, (_, on), nic in ids.inner[3][1] if not on][0] is True
    out = sc.run(sc.case("melody_outside_kit"))
    assert all(w[2] == sr.NO_MELODY for w in out.words[0]) and not any(out.inner[0]) and any(out.inner[2])
    nb = sc.run(sc.case("neighbouring_melodies"))
    assert len({w[2] for w in nb.words[0][:sc.K]}) == sc.K
    ov = sc.run(sc.case("overflow"))
    assert sum(sr.table(ov.inner[b], ov and sc.case("overflow").max_spans)[1] for b in range(sc.BUFFERS)) > 0
    off = sc.run(sc.case("note_off_first"))
    assert _stat("note_off_first", "resets") == n and off.words[0][0][2] == 0 and off.words[0][0][0] > 0   # melody 0 ran, no reset
    assert not sc.case("note_off_first").bank and all(c.bank for c in sc.CASES if c.name != "note_off_first")


@pytest.mark.parametrize("kind", sorted(sc.HOSTILE))
def test_hostile_rates_follow_the_arithmetic(kind):
    """the clock after a buffer at the hostile rate is what f32 makes of it, and the model goes on"""
    rec = sc.run(sc.case(f"rate_{kind}_held"))
    t1 = np.array([rec.words[1][0][1]], np.uint32).view(f32)[0]
    with np.errstate(all="ignore"):
        bt = f32(sc.OUT_LEN) / f32(sc.RATE)
        want = (f32(0) + bt) + f32(sc.OUT_LEN) / f32(sc.HOSTILE[kind])
    assert sr.bits(t1) == sr.bits(want)
    if kind == "zero":                                     # buf_time is infinite: the rest of the song falls into this one call
        assert rec.words[1][0][0] == len(sc.REFERENCE_MELODY) and np.isinf(t1)
    last = sc.run(sc.case(f"rate_{kind}")).words[-1][0]
    if kind == "nan":                                      # the re-press resets t to 0, the NaN buffer makes it NaN for good
        assert last[0] == 0 and np.isnan(np.array([last[1]], np.uint32).view(f32)[0])
    else:                                                  # after the re-press in buffer 1 the song runs again
        assert last[0] > 0
