"""The subsong tests' data, shared by tests/test_subsong_reference.py, tests/test_cpp_subsong.py, tests/test_gpu_subsong.py and
tests/test_gpu_subsong_player.py; holds no tests.  One kit of melodies (the reference's own from tests/golden/subsong_melody.json
beside synthetic ones) and a list of named cases; a case is a sample rate per buffer, a table capacity and a script of pushes
(frame, note_id, freq, note_on, melody) for every player over six consecutive buffers of 256 frames.  The sample rates are a few kHz,
so that the 0.1 s melody steps fall inside and across buffers.  The model (tests/subsong_reference.py) runs a case once for the
largest player count and every test slices what it needs -- player p's script does not depend on the player count.
A note-off is pushed under the id of the note it ends: a live voice bank routes it by that id, and the bare Trigger of the reference
reads nothing of a note-off's id that the stage uses."""
import functools
import json
import os
from dataclasses import dataclass

import numpy as np

from tests import subsong_reference as sr

f32 = np.float32
OUT_LEN = 256
BUFFERS = 6
PLAYERS = [1, 65, 130]
OUTER_SPANS = 34                                   # what zang_amd.subsong gives the outer bank
RATE = 2000.0                                      # a buffer is 0.128 s: the reference melody's 0.5 s end in the fourth
A4 = 440.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subsong_melody.json")


def semitone(s):
    return f32(A4 * 2.0 ** (s / 12.0))


def _reference_melody():
    g = json.load(open(GOLDEN))
    return [(f32(t), i, semitone(s), on) for t, i, s, on in zip(g["t"], g["note_id"], g["semitones_from_a4"], g["note_on"])], \
        semitone(g["base_semitones_from_a4"])


REFERENCE_MELODY, BASE_FREQ = _reference_melody()


CLAMP_CUTS = (2, 7)                                # the frames that cut buffer 0 of the "clamped" script: outer sub-spans [0, 2), [2, 7), ...


def clamp_time(rate=RATE):
    """a song time whose impulse NoteTracker.consume's @min (:180-183) has to clamp.  Right after a reset the clock t is the length
    of a short outer sub-span, [0, 2): t = 2 / rate.  The next sub-span, [2, 7), does not reset (a push under the same note id); its
    buf_time is 5 / rate and end_t = fl(t + buf_time).  For the largest f32 below end_t, note_t - t is not exact (t is less than half
    of note_t: Sterbenz's lemma does not apply) and rounds up to buf_time, so f is exactly 1 and f * out_len is out_len = 5, one
    past the sub-span: the impulse belongs on relative frame 4, frame 6 of the buffer.  Unclamped it would sit on the sub-span's
    end, where the Trigger's walk drops it while next_song_event has already moved on."""
    a, b = CLAMP_CUTS
    t0 = f32(0.0) + f32(a) / f32(rate)
    bt = f32(b - a) / f32(rate)
    end_t = t0 + bt
    note_t = np.nextafter(end_t, f32(0.0))
    assert t0 <= note_t < end_t and sr.int_from_float(((note_t - t0) / bt) * f32(b - a)) >= b - a
    return note_t


def last_frame_time(rate=RATE):
    """a song time that consume maps, unclamped, to the clamp's own value out_len - 1: the largest f32 below the end of buffer 1"""
    bt = f32(OUT_LEN) / f32(rate)
    t0 = f32(0.0) + bt
    end_t = t0 + bt
    note_t = np.nextafter(end_t, f32(0.0))
    assert note_t < end_t and sr.int_from_float(((note_t - t0) / bt) * f32(OUT_LEN)) == OUT_LEN - 1
    return note_t


M_REF, M_OFF_NEW_ID, M_PAIRS, M_DENSE, M_EMPTY, M_CLAMP, M_LAST = range(7)
KIT = [
    REFERENCE_MELODY,                                                                    # the note-off shares the last note-on's id
    REFERENCE_MELODY[:5] + [(REFERENCE_MELODY[5][0], 6) + REFERENCE_MELODY[5][2:]],      # ... and one where it does not
    [(f32(0.05), 1, semitone(-9), True), (f32(0.05), 2, semitone(-2), True),             # two events at one time: one frame
     (f32(0.2), 3, semitone(-5), True), (f32(0.2), 3, semitone(-5), False)],
    [(f32(0.002 * i), i // 2 + 1, semitone(-9 + i % 12), i % 2 == 0) for i in range(100)],  # 4 frames apart at RATE: more than 32 a call, twice
    [],
    [(f32(0.0), 1, semitone(-9), True), (clamp_time(), 2, semitone(-4), True)],
    [(f32(0.0), 1, semitone(-9), True), (last_frame_time(), 2, semitone(-4), True)],
]
K = len(KIT)


@dataclass(frozen=True)
class Case:
    name: str
    script: str                                    # which of the scripts below
    max_spans: int = 66
    rates: tuple = (RATE,) * BUFFERS               # the sample rate of each buffer
    bank: bool = True                              # False: the outer table cannot come out of a voice bank's dispatcher

    def rate(self, b):
        return self.rates[b]


def key_freq(p):
    """player p's key: around a4, most players inside the oscillator's range at RATE (freq * melody / base <= RATE / 8)"""
    return f32(110.0 + 7.0 * (p % 9))


def _shift(p):
    return (p * 5) % 23


def script(case, p):
    """-> per buffer, player p's pushes [(frame, note_id, freq, note_on, melody)] in push order (frames ascending)"""
    kf, d = key_freq(p), _shift(p)
    out = [[] for _ in range(BUFFERS)]
    s = case.script
    if s == "held":                                # the reference melody held to its end
        out[0] = [(0, 1, kf, True, M_REF)]
    elif s == "release":                           # a release mid-melody: the melody goes on, no reset
        out[0] = [(d, 1, kf, True, M_REF)]
        out[1] = [(40 + d, 1, kf, False, M_REF)]
    elif s == "repress":                           # a re-press mid-melody: reset
        out[0] = [(d, 1, kf, True, M_REF)]
        out[1] = [(90 + d, 2, f32(kf * f32(1.25)), True, M_OFF_NEW_ID)]
        out[4] = [(255, 2, f32(kf * f32(1.25)), False, M_REF)]
    elif s == "two_presses":                       # two presses in one buffer: two resets
        out[0] = [(10 + d, 1, kf, True, M_REF), (150 + d, 2, f32(kf * f32(1.5)), True, M_PAIRS)]
        out[2] = [(0, 3, kf, True, M_DENSE), (0, 4, kf, True, M_REF)]          # ... and two at one frame
    elif s == "key_change":                        # the key's frequency changes under the SAME note id while an inner note is carried
        out[0] = [(0, 1, kf, True, M_REF)]
        out[1] = [(100 + d, 1, f32(kf * f32(1.5)), True, M_REF)]
        out[2] = [(33, 1, f32(kf * f32(0.75)), True, M_REF)]
    elif s == "uneven_cut":                        # held, with buffer 1 cut at 7 and 36 by pushes that change nothing: 7 / RATE +
        out[0] = [(0, 1, kf, True, M_REF)]         # 29 / RATE + 220 / RATE summed onto t in f32 is not 256 / RATE summed onto it
        out[1] = [(7, 1, kf, True, M_REF), (36, 1, kf, True, M_REF)]
    elif s == "one_frame":                         # an outer sub-span of one frame
        out[0] = [(0, 1, kf, True, M_REF)]
        out[1] = [(100 + d, 1, kf, True, M_REF), (101 + d, 1, kf, True, M_REF)]
        out[2] = [(255, 2, kf, True, M_PAIRS)]                                 # ... and a press on a buffer's last frame
    elif s == "clamped":                           # an impulse clamped to out_len - 1 (clamp_time): pushes under ONE id cut buffer 0
        out[0] = [(0, 1, kf, True, M_CLAMP)] + [(c, 1, kf, True, M_CLAMP) for c in CLAMP_CUTS]
    elif s == "last_frame":                        # an impulse that lands on out_len - 1 of itself (last_frame_time)
        out[0] = [(0, 1, kf, True, M_LAST)]
    elif s == "pairs":                             # two song events on the same frame
        out[0] = [(d, 1, kf, True, M_PAIRS)]
        out[3] = [(d, 2, kf, True, M_PAIRS)]
    elif s == "dense":                             # more than 32 events inside one sub-span
        out[0] = [(d, 1, kf, True, M_DENSE)]
        out[2] = [(0, 2, kf, True, M_DENSE)]
    elif s == "off_ids":                           # the note-off shares its note-on's id (even players) or does not (odd)
        out[0] = [(0, 1, kf, True, M_REF if p % 2 == 0 else M_OFF_NEW_ID)]
    elif s == "outside":                           # a melody index at or above K
        out[0] = [(d, 1, kf, True, [K, K + 1, 0xffffffff][p % 3])]
        out[2] = [(d, 2, kf, True, M_REF)]
        out[3] = [(d, 3, kf, True, K)]
    elif s == "off_first":                         # an outer note-off with no earlier note-on: melody 0 from its start, no reset
        out[0] = [(30 + d, 1, kf, False, M_PAIRS)]
        out[2] = [(d, 2, kf, True, M_PAIRS)]
    elif s == "neighbours":                        # different melodies on neighbouring players
        out[0] = [(d, 1, kf, True, p % K)]
        out[3] = [(200 - d, 2, f32(kf * f32(2.0)), True, (p + 3) % K)]
    else:
        raise ValueError(s)
    return out


HOSTILE = {"zero": 0.0, "negative": -2000.0, "nan": float("nan"), "inf": float("inf")}


def _hostile_rates(x):
    return (RATE, x, RATE, RATE, x, RATE)          # buffers 1 and 4 run at the hostile rate; "repress" resets in buffer 1


CASES = [
    Case("reference_melody_held", "held"),
    Case("release_mid_melody", "release"),
    Case("repress_mid_melody", "repress"),
    Case("two_presses_one_buffer", "two_presses"),
    Case("key_change_carried_note", "key_change"),
    Case("uneven_outer_cut", "uneven_cut"),
    Case("one_frame_outer", "one_frame"),
    Case("clamped_impulse", "clamped"),
    Case("last_frame_impulse", "last_frame"),
    Case("same_frame_events", "pairs"),
    Case("more_than_32_events", "dense"),
    Case("note_off_ids", "off_ids"),
    Case("melody_outside_kit", "outside"),
    Case("neighbouring_melodies", "neighbours"),
    Case("overflow", "dense", max_spans=3),
    Case("note_off_first", "off_first", bank=False),
] + [Case(f"rate_{k}", "repress", rates=_hostile_rates(v)) for k, v in HOSTILE.items()] \
  + [Case(f"rate_{k}_held", "held", rates=_hostile_rates(v)) for k, v in HOSTILE.items()]
CASE_IDS = [c.name for c in CASES]
BANK_CASES = [c for c in CASES if c.bank]          # what a test that pushes into a live voice bank runs
BANK_CASE_IDS = [c.name for c in BANK_CASES]


def case(name):
    return next(c for c in CASES if c.name == name)


@dataclass
class Run:
    """the model's record of one case: per buffer and player the outer and the inner sub-spans and the state words after it"""
    outer: list                                    # [buffer][player] -> [(s, e, (freq, note_on, melody), changed)]
    inner: list                                    # [buffer][player] -> [(s, e, (freq, note_on), changed)]
    words: list                                    # [buffer][player] -> zh_subsong_state's fields, t and freq as bits
    stats: list                                    # [player] -> the model's counters at the end


@functools.lru_cache(maxsize=None)
def run(case, n_players=max(PLAYERS)):
    players = [sr.Player(KIT, BASE_FREQ) for _ in range(n_players)]
    scripts = [script(case, p) for p in range(n_players)]
    rec = Run([], [], [], [])
    for b in range(BUFFERS):
        outer, inner, words = [], [], []
        for p, pl in enumerate(players):
            for ev in scripts[p][b]:
                pl.push(*ev)
            o, i = pl.schedule(OUT_LEN, case.rate(b))
            outer.append(o); inner.append(i); words.append(pl.player.words())
        rec.outer.append(outer); rec.inner.append(inner); rec.words.append(words)
    rec.stats = [pl.stats() for pl in players]
    return rec


INIT_WORDS = [0, 0, 0, 0, 0, 0, 0]                 # init(): everything zero, the melody 0


def state_array(words, dtype):
    """[player] word lists -> a zh_subsong_state array (t and freq from their bits)"""
    st = np.zeros(len(words), dtype)
    for p, w in enumerate(words):
        st["next_song_event"][p], st["melody"][p], st["has_note"][p], st["note_id"][p], st["note_on"][p] = w[0], w[2], w[3], w[4], w[6]
        st["t"][p] = np.array([w[1]], np.uint32).view(f32)[0]
        st["freq"][p] = np.array([w[5]], np.uint32).view(f32)[0]
    return st


def state_words(st):
    """a zh_subsong_state array -> [player] word lists"""
    return [[int(st["next_song_event"][p]), int(st["t"][p:p + 1].view(np.uint32)[0]), int(st["melody"][p]), int(st["has_note"][p]),
             int(st["note_id"][p]), int(st["freq"][p:p + 1].view(np.uint32)[0]), int(st["note_on"][p])] for p in range(len(st))]
