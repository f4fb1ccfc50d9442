"""The case list of the merge-stage tests (tests/test_two_reference.py, test_cpp_two.py, test_gpu_span_merge.py); holds no tests.
A case is one player's two source row lists and, for the hand-written ones, the merged rows written out by hand from
examples/example_two.zig:93-151.  Source rows: (start, end, note_id_changed, words); merged rows: (start, end, note_id_changed,
A's words + B's words + [note_on, nic_a, nic_b]).  The default shape is the example's: A = {freq f, note_on u}, B = {color f,
note_on u}; WIDE has four fields and one, with the note-on first."""
from collections import namedtuple

import numpy as np

OUT_LEN = 256
SOURCE_SPANS = 34
MAX_SPANS = 67
PLAYERS = 66                                       # the CPU harness: crosses a wave edge
Shape = namedtuple("Shape", "kinds_a on_a kinds_b on_b")
EXAMPLE = Shape("fu", 1, "fu", 1)
WIDE = Shape("uffu", 0, "u", 0)
Case = namedtuple("Case", "name a b expect")


def fb(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


F1, F2, F3 = fb(440.0), fb(660.0), fb(220.0)
C1, C2 = fb(0.5), fb(0.853553)

# (a) B's row ends inside A's: A's nic stays set on BOTH merged rows; the envelope restarts on both (B's nic is off)
STICKY = Case("sticky_nic",
              [(0, 256, 1, (F1, 1))],
              [(0, 100, 0, (C1, 0)), (100, 256, 0, (C2, 0))],
              [(0, 100, 1, [F1, 1, C1, 0, 1, 1, 0]), (100, 256, 1, [F1, 1, C2, 0, 1, 1, 0])])
# ... and where B's second row is a new note-on too, each masks the other: no restart, with both nics set
STICKY_MASKED = Case("sticky_nic_masked",
                     [(0, 256, 1, (F1, 1))],
                     [(0, 100, 0, (C1, 0)), (100, 256, 1, (C2, 1))],
                     [(0, 100, 1, [F1, 1, C1, 0, 1, 1, 0]), (100, 256, 0, [F1, 1, C2, 1, 1, 1, 1])])
# both end at 100: both advance, two rows
TIE = Case("tie_both_advance",
           [(0, 100, 1, (F1, 1)), (100, 256, 1, (F2, 0))],
           [(0, 100, 0, (C1, 0)), (100, 256, 1, (C2, 1))],
           [(0, 100, 1, [F1, 1, C1, 0, 1, 1, 0]), (100, 256, 0, [F2, 0, C2, 1, 1, 1, 1])])
# a source without a row: nothing
EMPTY_A = Case("empty_source_a", [], [(0, 256, 1, (C1, 1))], [])
EMPTY_B = Case("empty_source_b", [(0, 256, 1, (F1, 1))], [], [])
# (b) A's first row starts at 50; starts are never read: merged from frame 0 with that row's values
LATE = Case("late_first_row",
            [(50, 256, 1, (F3, 1))],
            [(0, 256, 0, (C1, 0))],
            [(0, 256, 1, [F3, 1, C1, 0, 1, 1, 0])])
# (c) A runs out at 100: nothing follows, B's rows to 256 are left
RUNS_OUT = Case("source_runs_out",
                [(0, 100, 0, (F1, 0))],
                [(0, 60, 1, (C1, 1)), (60, 256, 0, (C2, 0))],
                [(0, 60, 1, [F1, 0, C1, 1, 1, 0, 1]), (60, 100, 0, [F1, 0, C2, 0, 0, 0, 0])])
# an end at or below the position ends the list; so does an end above out_len
BACKWARDS = Case("malformed_end_backwards",
                 [(0, 100, 1, (F1, 1)), (100, 90, 1, (F2, 1)), (90, 256, 1, (F3, 1))],
                 [(0, 256, 0, (C1, 0))],
                 [(0, 100, 1, [F1, 1, C1, 0, 1, 1, 0])])
EMPTY_ROW = Case("malformed_end_empty_row",
                 [(0, 100, 1, (F1, 1)), (100, 100, 1, (F2, 1)), (100, 256, 1, (F3, 1))],
                 [(0, 256, 0, (C1, 0))],
                 [(0, 100, 1, [F1, 1, C1, 0, 1, 1, 0])])
TOO_LONG = Case("malformed_end_past_out_len",
                [(0, 100, 1, (F1, 1)), (100, 300, 0, (F2, 1))],
                [(0, 100, 0, (C1, 0)), (100, 257, 0, (C2, 0))],
                [(0, 100, 1, [F1, 1, C1, 0, 1, 1, 0])])
# a note-off with nic set restarts nothing; note_on is the OR
NOTE_OFFS = Case("note_offs",
                 [(0, 40, 1, (F1, 0)), (40, 256, 1, (F2, 1))],
                 [(0, 256, 1, (C1, 0))],
                 [(0, 40, 0, [F1, 0, C1, 0, 0, 1, 1]), (40, 256, 0, [F2, 1, C1, 0, 1, 1, 1])])
HAND = [STICKY, STICKY_MASKED, TIE, EMPTY_A, EMPTY_B, LATE, RUNS_OUT, BACKWARDS, EMPTY_ROW, TOO_LONG, NOTE_OFFS]
HAND_IDS = [c.name for c in HAND]


def random_rows(rng, kinds, on, full):
    """up to 34 rows cut at sorted distinct frames of (0, 256]; `full`: the last row ends at 256, else the source may run out
    early; a first row that starts late now and then; values random, note-on words 0 / 1 and now and then another non-zero word"""
    n = int(rng.integers(1, SOURCE_SPANS + 1))
    ends = np.sort(rng.choice(np.arange(1, OUT_LEN + 1), n, replace=False)).tolist()
    if full:
        ends[-1] = OUT_LEN
    rows, pos = [], int(rng.integers(0, ends[0])) if rng.random() < 0.2 else 0
    for e in ends:
        words = [int(rng.integers(0, 1 << 32)) if k == "f" else int(rng.integers(0, 5)) for k in kinds]
        words[on] = int(rng.choice([0, 1, 1, 0x100]))
        rows.append((pos, e, int(rng.random() < 0.5), tuple(words)))
        pos = e
    return rows


def widen(rows, kinds, on):
    """an EXAMPLE-shaped source's rows in another shape: the note-on word moves to `on`, the first word to the first other field,
    the rest is filled from the row's end"""
    out = []
    for s, e, nic, w in rows:
        words = [(e * 2654435761 + 97 * i) & 0xffffffff for i in range(len(kinds))]
        words[on] = w[1]
        others = [i for i in range(len(kinds)) if i != on]
        if others:
            words[others[0]] = w[0]
        out.append((s, e, nic, tuple(words)))
    return out


def players(n, shape=EXAMPLE, seed=20260121):
    """n players' sources: the hand-written cases first (in `shape`), then random ones, some of which tie often (both sources cut
    from one grid).  -> (players_a, players_b)"""
    rng = np.random.default_rng(seed)
    pa, pb = [], []
    for p in range(n):
        if p < len(HAND):
            a, b = HAND[p].a, HAND[p].b
            if shape != EXAMPLE:
                a, b = widen(a, shape.kinds_a, shape.on_a), widen(b, shape.kinds_b, shape.on_b)
        else:
            a = random_rows(rng, shape.kinds_a, shape.on_a, full=p % 3 != 0)
            b = random_rows(rng, shape.kinds_b, shape.on_b, full=p % 5 != 0)
            if p % 4 == 1:                                         # ties: B's ends are a subset of A's, plus the last
                keep = [r for r in a if rng.random() < 0.6] or a[:1]
                b = [(0 if i == 0 else keep[i - 1][1], r[1], b[i % len(b)][2], b[i % len(b)][3]) for i, r in enumerate(keep)]
        pa.append(a)
        pb.append(b)
    return pa, pb


OVERFLOW_MAX_SPANS = (1, 5)                        # the hand cases make up to 2 rows, random ones up to 67
