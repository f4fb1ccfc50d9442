"""CPU: facts of the polyphony model (tests/polyphony_reference.py) that can be read off examples/example_polyphony.zig by hand,
and of the case list (tests/polyphony_cases.py): the model is the yardstick of the key fan-out stage's tests, so what it says
about the simplest key presses is checked against the Zig here, without the stage."""
import numpy as np
import pytest

from tests import polyphony_cases as pc
from tests import polyphony_reference as pr

KEYS = pc.CASES[0].key_freqs()


def _buffer(m, events):
    for key, down, frame in events:
        m.key_event(key, down, frame)
    return m.schedule(pc.OUT_LEN)[1]


def test_a_press_at_frame_100_and_the_buffer_after_it():
    m = pr.MainModule(KEYS)
    inner = _buffer(m, [(7, True, 100)])
    assert inner[7] == [(100, 256, (KEYS[7], True), True)]                    # the key's first note: changed
    assert all(not spans for k, spans in enumerate(inner) if k != 7)           # no other key has a note to carry
    inner = _buffer(m, [])
    assert inner[7] == [(0, 256, (KEYS[7], True), False)]                      # carried: one outer sub-span, nothing new
    assert all(not spans for k, spans in enumerate(inner) if k != 7)


def test_another_keys_event_splits_the_held_keys_row():
    m = pr.MainModule(KEYS)
    _buffer(m, [(7, True, 0)])
    inner = _buffer(m, [(9, True, 50)])
    assert inner[7] == [(0, 50, (KEYS[7], True), False), (50, 256, (KEYS[7], True), False)]
    assert inner[9] == [(50, 256, (KEYS[9], True), True)]


def test_a_release_is_a_note_off_with_a_fresh_id():
    m = pr.MainModule(KEYS)
    _buffer(m, [(7, True, 0)])
    assert m.polyphony.voices[7].words()[:4] == [2, 1, 1, 1]                   # next_id, down, has_note, note_id
    inner = _buffer(m, [(7, False, 10)])
    assert inner[7] == [(0, 10, (KEYS[7], True), False), (10, 256, (KEYS[7], False), True)]
    assert m.polyphony.voices[7].words() == [3, 0, 1, 2, pr.bits(KEYS[7]), 0]
    assert m.polyphony.voices[8].words() == [1, 0, 0, 0, 0, 0]                 # Voice :50-56


def test_every_key_event_pushes_the_whole_mask_with_a_fresh_id():
    m = pr.MainModule(KEYS)
    assert m.key_event(3, True, 5) == (1, 8) and m.key_event(40, True, 5) == (2, 8 | 1 << 40) and m.key_event(3, False, 9) == (3, 1 << 40)


def test_the_space_bar_cycles_seven_modes():
    m = pr.MainModule(KEYS)
    assert [m.space() for _ in range(8)] == [1, 2, 3, 4, 5, 6, 0, 1] and pr.DEC_RATES[1:] == (6000.0, 5000.0, 4000.0, 3000.0, 2000.0, 1000.0)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_the_cases_reach_what_they_are_for(case):
    rec = pc.run(case)
    K = case.n_keys
    assert all(len(rec.pushed[4][p]) == 33 and len(rec.outer[4][p]) <= 33 for p in range(pc.PLAYERS))       # the queue dropped one
    assert any(len(o) == 33 for o in rec.outer[4])                             # the carried note + 32 impulses
    assert all(len(rec.outer[3][p]) == 3 for p in range(pc.PLAYERS))           # [0, 77) carried, the second impulse of frame 77, 255
    assert [s for s, _, _, _ in rec.outer[0][0]] == [0] and [s for s, _, _, _ in rec.outer[0][1]] == [100]
    if K > 1:
        assert rec.inner[1][0][:3] == [(0, 50, (case.key_freqs()[0], True), False), (50, 120, (case.key_freqs()[0], True), False),
                                       (120, 256, (case.key_freqs()[0], True), False)]
    _, dropped = pr.table(rec.inner[1], case.max_spans)
    assert (dropped > 0) == (case.name == "overflow")
    assert max(len(s) for b in range(pc.BUFFERS) for s in rec.inner[b]) <= 34
    if case.stray:                                                             # the stray bits are in the records and in no voice
        assert all(m & case.stray == case.stray for b in rec.pushed for p in b for _, _, m in p)
        assert len(rec.inner[0]) == pc.PLAYERS * K
    ids = np.array([w[0] for w in rec.words[-1]])
    assert ids.max() > 3 and ids.min() >= 1
