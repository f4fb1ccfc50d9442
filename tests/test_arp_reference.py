"""CPU: the arpeggiator model (tests/arp_reference.py) against answers derived by hand from examples/example_arpeggiator.zig and
src/zang/trigger.zig, and the case list (tests/arp_cases.py) against what it claims to cover."""
import numpy as np
import pytest

from tests import arp_cases as ac
from tests import arp_reference as ar

F = [np.float32(x) for x in (100.0, 200.0, 300.0, 400.0)]
OUT = 256


def _buffer(pl, events, sample_rate):
    for key, down, frame in events:
        pl.key_event(key, down, frame)
    return pl.schedule(OUT, sample_rate)[1]


def test_one_key_held_from_frame_zero_with_a_note_longer_than_the_buffer():
    """note_duration 300 (0.03f * 10001 = 300.03): one tick per buffer at most.  Buffer 0: the tick at 0, id 1, the clock goes to
    300 - 256 = 44.  Buffer 1: the carried note to 44, then the SAME key again under a fresh id (the search from key 3 wraps to key
    2), 44 + 300 - 256 = 88.  Buffer 2 likewise at 88."""
    pl = ar.Player(F)
    assert ar.note_duration(10001.0) == 300
    assert _buffer(pl, [(2, True, 0)], 10001.0) == [(0, 256, (F[2], True), True)]
    assert pl.arp.words()[:5] == [44, 2, 2, 1, 1]
    assert _buffer(pl, [], 10001.0) == [(0, 44, (F[2], True), False), (44, 256, (F[2], True), True)]
    assert pl.arp.words()[:5] == [88, 3, 2, 1, 2]
    assert _buffer(pl, [], 10001.0) == [(0, 88, (F[2], True), False), (88, 256, (F[2], True), True)]
    assert pl.arp.words()[:5] == [132, 4, 2, 1, 3]


def _three_keys():
    """three keys down at frame 0 (the outer Trigger skips the first two impulses: the next one starts at the same frame), two
    buffers at note_duration 100: ticks 0, 100, 200 then 44, 144, 244, lowest key to highest and round again"""
    pl = ar.Player(F[:3])
    assert ar.note_duration(3334.0) == 100
    got = _buffer(pl, [(0, True, 0), (1, True, 0), (2, True, 0)], 3334.0)
    assert got == [(0, 100, (F[0], True), True), (100, 200, (F[1], True), True), (200, 256, (F[2], True), True)]
    assert pl.arp.words()[:5] == [44, 4, 2, 1, 3]
    got = _buffer(pl, [], 3334.0)
    assert got == [(0, 44, (F[2], True), False), (44, 144, (F[0], True), True), (144, 244, (F[1], True), True), (244, 256, (F[2], True), True)]
    assert pl.arp.words()[:5] == [88, 7, 2, 1, 6]
    return pl


def test_three_keys_cycle_lowest_to_highest():
    _three_keys()


def test_release_of_all_keys_sends_note_offs_at_the_last_keys_frequency():
    """after the two buffers above, all three keys go up at frame 50.  Outer: [0, 50) with the keys held, [50, 256) with none.
    Call 1 ticks at 88 and 188 (keys 0, 1; ids 7, 8): both lie at or above 50, so the carried key 2 plays to 50 and they are lost,
    yet last_note is 1 and the clock moved a buffer (288 - 256 = 32).  Call 2 ticks at 32, 132, 232: no key is held, so each is a
    note-off at key 1's frequency (ids 9, 10, 11); the one at 32 lies below the walk's position 50 and is taken there."""
    pl = _three_keys()
    got = _buffer(pl, [(0, False, 50), (1, False, 50), (2, False, 50)], 3334.0)
    assert got == [(0, 50, (F[2], True), False), (50, 132, (F[1], False), True), (132, 232, (F[1], False), True), (232, 256, (F[1], False), True)]
    assert pl.arp.words() == [76, 12, 1, 1, 11, int(np.array([F[1]]).view(np.uint32)[0]), 0]
    assert pl.arp.stats["at_or_above_end"] == 2 and pl.arp.stats["below_start"] == 1


def test_a_key_event_mid_buffer_doubles_the_clock_step():
    """key 0 down at 0 (buffer 0: ticks 0, 100, 200; clock 44), key 1 down at 128 in buffer 1.  Two outer sub-spans, two calls,
    and `next_frame -= out_len` in each: call 1 ticks 44, 144, 244 (clock 88), call 2 ticks 88, 188 (clock 32) -- two buffers'
    worth in one.  Call 1 walks [0, 128): the tick at 144 ends it.  Call 2 walks [128, 256): its tick at 88 is taken at 128."""
    pl = ar.Player(F[:2])
    _buffer(pl, [(0, True, 0)], 3334.0)
    assert pl.arp.words()[:5] == [44, 4, 0, 1, 3]
    got = _buffer(pl, [(1, True, 128)], 3334.0)
    assert got == [(0, 44, (F[0], True), False), (44, 128, (F[0], True), True), (128, 188, (F[1], True), True), (188, 256, (F[0], True), True)]
    assert pl.arp.words()[:5] == [32, 9, 0, 1, 8]


def test_nothing_runs_before_the_first_key_event():
    pl = ar.Player(F)
    assert _buffer(pl, [], 3334.0) == [] and pl.arp.words() == [0, 1, -1, 0, 0, 0, 0] and pl.arp.stats["calls"] == 0


def test_the_f32_rate_is_what_the_search_finds():
    assert ac.search_f32_rate() == ac.F32_RATE
    assert ar.note_duration(ac.F32_RATE) == 87 and ar.note_duration_f64(ac.F32_RATE) == 86


@pytest.mark.parametrize("rate", ac.REJECTED_RATES, ids=[str(r) for r in ac.REJECTED_RATES])
def test_rejected_rates(rate):
    assert ar.note_duration(rate) is None


def test_note_durations_of_the_cases():
    assert {c.name: c.note_duration for c in ac.CASES} == ac.EXPECTED_ND
    assert {c.n_keys for c in ac.CASES} == {1, 39, 64}


@pytest.mark.parametrize("case", ac.CASES, ids=ac.CASE_IDS)
def test_what_every_case_covers(case):
    """the model itself reports: a generated frame below the outer sub-span's start and one at or above its end; per buffer 0 to
    max_events key events, at frames 0 and out_len - 1 and at equal frames; keys 0 and n_keys - 1; a buffer after all keys were
    released that still plays (note-offs); players with no rows in buffer 0"""
    rec = ac.run(case)
    N = len(rec.stats)
    assert sum(s["below_start"] for s in rec.stats) > 0 and sum(s["at_or_above_end"] for s in rec.stats) > 0
    scripts = [ac.script(case, p) for p in range(N)]
    counts = {len(evs) for sc in scripts for b, evs in enumerate(sc) if b != 3}
    assert counts >= set(range(case.max_events + 1)), counts
    frames = [[f for _, _, f in evs] for sc in scripts for evs in sc]
    assert any(0 in fr for fr in frames) and any(ac.OUT_LEN - 1 in fr for fr in frames) and any(len(set(fr)) < len(fr) for fr in frames)
    keys = {k for sc in scripts for evs in sc for k, _, _ in evs}
    assert {0, case.n_keys - 1} <= keys
    assert any(not rec.inner[0][p] and rec.words[0][p] == [0, 1, -1, 0, 0, 0, 0] for p in range(N))
    offs = [sp for p in range(N) for sp in rec.inner[4][p] if not sp[2][1]]
    assert offs, "no note-off after the release of all keys"
    if case.note_duration <= 7:                                      # more than 32 ticks in one call: pushes dropped, ids still drawn
        assert sum(s["dropped_pushes"] for s in rec.stats) > 0
    if case.name == "overflow":
        assert sum(ar.table(rec.inner[b], case.max_spans)[1] for b in range(ac.BUFFERS)) > 0
    else:
        assert all(ar.table(rec.inner[b], case.max_spans)[1] == 0 for b in range(ac.BUFFERS))
    assert all(len(o) <= ac.OUTER_SPANS for b in range(ac.BUFFERS) for o in rec.outer[b])


def test_ids_advance_past_the_queues_cap():
    """note_duration 1, one key: 256 ticks in the first call, 32 accepted -- next_id is 257 all the same"""
    pl = ar.Player(F[:1])
    got = _buffer(pl, [(0, True, 0)], 40.0)
    assert len(got) == 32 and got[-1][:2] == (31, 256) and pl.arp.words()[:5] == [0, 257, 0, 1, 32]
