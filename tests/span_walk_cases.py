"""The edge rules of the Trigger sub-span walk (csrc/span_walk.hip.h) as data: one small table per rule, a plain-Python model of
the walk, and the per-voice arrays the span paints take.  Shared by tests/test_gpu_span_walk_edges.py; nothing here needs a GPU.

Geometry: an image of IMG_F frames painted over [BUF_START, BUF_END) -- the buffer starts after frame 0 and ends before the
image does, so a walk that strays outside the paint span shows in the image."""
import numpy as np

IMG_F = 128
BUF_START, BUF_END = 8, 104
K = 3                                    # max_spans of every table here
ROWS = K + 1                             # rows the arrays really have: a walker that does not clip count to max_spans reads row K

# (what the case pins, [(start, end), ...], count -- None: len(spans)).  Voice v of a paint takes case (offset + v) % len(CASES).
CASES = [
    ("three adjacent sub-spans, the first at buf_start, the last ending at buf_end", [(8, 40), (40, 72), (72, 104)], None),
    ("one sub-span equal to the paint span", [(8, 104)], None),
    ("lengths 1, 7 and 8", [(10, 11), (20, 27), (30, 38)], None),
    ("lengths 9 and 63", [(9, 18), (21, 84)], None),
    ("length 64", [(13, 77)], None),
    ("length 65", [(11, 76)], None),
    ("an empty sub-span mid-buffer, then one that starts at the same frame", [(50, 50), (50, 70)], None),
    ("s == e == buf_end: prologue and epilogue, no frame", [(20, 30), (104, 104)], None),
    ("s == buf_end, e > buf_end: prologue only", [(104, 120)], None),
    ("a first entry with s < buf_start: nothing fires", [(4, 20), (30, 40)], None),
    ("a second entry that starts inside the first: the first runs and ends, nothing after it fires", [(10, 30), (25, 50), (60, 70)], None),
    ("e < s: runs to buf_end, no epilogue, nothing after it", [(40, 20), (60, 70)], None),
    ("e > buf_end: runs to buf_end, no epilogue", [(40, 110), (112, 120)], None),
    ("s > buf_end: never reached", [(10, 20), (110, 120)], None),
    ("count > max_spans: clipped to max_spans (row K holds an entry that would fire)", [(8, 20), (20, 30), (40, 50), (60, 70)], None),
    ("count == 0", [], None),
]


def trigger_calls(spans, count, K, buf_start, buf_end):
    """The paint calls the walk makes for one voice over [buf_start, buf_end) -> [(k, s, e_painted, ended)]: sub-span k begins
    (prologue) at s, paints [s, e_painted), and `ended` says whether its epilogue runs.  The contract of csrc/span_walk.hip.h: an
    entry that starts before the previous one ended, before buf_start or after buf_end is never reached and ends the list; one
    that ends before it starts or after buf_end runs to buf_end without its epilogue (and nothing follows it)."""
    calls, i = [], buf_start
    for k in range(min(count, K)):
        s, e = spans[k][0], spans[k][1]
        if s < i or s > buf_end:
            break
        ended = s <= e <= buf_end
        calls.append((k, s, e if ended else buf_end, ended))
        if not ended:
            break
        i = e
    return calls


def case_of(v, offset=0):
    return CASES[(offset + v) % len(CASES)]


def tables(V, offset=0):
    """-> dict of host arrays: count [V] u32; start / end [ROWS][V] u32; freq [ROWS][V] f32; note_on / note_id_changed [ROWS][V] u8
    (one row more than the max_spans = K the paints are given).
    Every first sub-span is a new note, the second releases it, the third is a new note again (so every case has a sub-span with
    note_id_changed set, and no note comes back on without a new id)."""
    tb = {"count": np.zeros(V, np.uint32), "start": np.zeros((ROWS, V), np.uint32), "end": np.zeros((ROWS, V), np.uint32),
          "freq": np.zeros((ROWS, V), np.float32), "note_on": np.zeros((ROWS, V), np.uint8), "note_id_changed": np.zeros((ROWS, V), np.uint8)}
    for v in range(V):
        _, spans, count = case_of(v, offset)
        tb["count"][v] = len(spans) if count is None else count
        for k, (s, e) in enumerate(spans):
            tb["start"][k, v], tb["end"][k, v] = s, e
            tb["freq"][k, v] = 180.0 * (1.0 + 0.37 * k) * (1.0 + 0.021 * v)
            tb["note_on"][k, v] = k != 1
            tb["note_id_changed"][k, v] = k != 1
    return tb


def calls(tb, v):
    """trigger_calls of voice v of tables()"""
    spans = [(int(tb["start"][k, v]), int(tb["end"][k, v])) for k in range(ROWS)]
    return trigger_calls(spans, int(tb["count"][v]), K, BUF_START, BUF_END)


def all_ended(tb, V):
    """voices whose every reached sub-span ended: their state is the oracle's (its paint always runs the epilogue)"""
    return np.array([all(c[3] for c in calls(tb, v)) for v in range(V)], bool)


OFFSETS_FOR = {3: tuple(range(0, len(CASES), 3)), 65: (0,)}      # V -> the offsets at which V voices reach every case
