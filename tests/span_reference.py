"""The shared pieces of the *_reference.py and *_cases.py yardsticks; holds no tests.  What every voice's model of correctness
has in common stands here once: the span paints' walk contract (walk), a sub-span's field or its default (value), the reference's
ImpulseQueue (src/zang/notes.zig:72-128) and Trigger (src/zang/trigger.zig:26-198) restated from the Zig alone, the span-table
stages' table and its comparison (table, same_table), and a voice's state as uint32 words (state_words, struct_state, same_words).
A voice's own file keeps its oracle calls, its fields and its STATE description, and imports the rest from here."""
import numpy as np

f32 = np.float32
MAX_IMPULSES = 32                                  # notes.zig:73


def bits(x):
    """an f32's bits"""
    return int(np.array([x], f32).view(np.uint32)[0])


# ---- the span paints' contract
def walk(tb, v, S, E):
    """the rows of voice v a span paint reaches, under the span paints' contract: the first min(count, K); a row that starts
    before the previous one ends, before S or after E ends the list -> [(k, start, end)]"""
    out, i = [], S
    for k in range(min(int(tb["count"][v]), tb["start"].shape[0])):
        s, e = int(tb["start"][k, v]), int(tb["end"][k, v])
        if s < i or s > E:
            break
        assert s <= e <= E
        out.append((k, s, e))
        i = e
    return out


def value(tb, dflt, name, k, v):
    """field `name` of sub-span k, voice v: the table's array, else the per-voice / broadcast default"""
    if tb.get(name) is not None:
        return tb[name][k, v]
    d = dflt[name]
    return d[v] if isinstance(d, np.ndarray) else d


# ---- the reference's host side
class ImpulseQueue:
    """notes.zig:72-128: push drops at 32 and on a frame below the last accepted one's; consume empties.  Impulses are stored in
    a list, as the reference stores them in its arrays of 32."""

    def __init__(self):
        self.items = []                            # (frame, note_id, params)

    def push(self, frame, note_id, params):
        if len(self.items) >= MAX_IMPULSES:        # :108-111
            return
        if self.items and frame < self.items[-1][0]:   # :112-118
            return
        self.items.append((frame, note_id, params))

    def consume(self):
        items, self.items = self.items, []
        return items


class Trigger:
    """trigger.zig:26-198; `note` = (id, params) or None.  counter() + next() as the reference has them: next -> (start, end,
    params, note_id_changed) or None, one sub-span per call; spans() is the loop over next.  Where the reference is undefined: an
    impulse below the Trigger's position (its assert, :161) is taken at the position."""

    def __init__(self):
        self.note = None

    def reset(self):                                                           # :58-60
        self.note = None

    def counter(self, start, end, impulses):                                   # :62-70
        return {"pos": start, "end": end, "impulses": impulses, "idx": 0}

    def next(self, ctr):                                                       # :80-105
        imp = ctr["impulses"]
        while ctr["pos"] < ctr["end"]:                                         # :81
            pos, end, span = ctr["pos"], ctr["end"], None
            if self.note is not None:                                          # carryOver :107-137
                if ctr["idx"] < len(imp):
                    nf = imp[ctr["idx"]][0]
                    if nf > pos:
                        span = (pos, min(end, nf), self.note)
                else:
                    span = (pos, end, self.note)
            if span is None:                                                   # getNextNoteSpan :139-196
                span = (pos, end, None)
                while ctr["idx"] < len(imp):
                    frame, note_id, params = imp[ctr["idx"]]
                    if frame >= end:                                           # :144-150
                        break
                    if frame > pos:                                            # :152-159
                        span = (pos, frame, None)
                        break
                    ctr["idx"] += 1                                            # :163 (:161 asserts frame == pos; below: taken here)
                    clipped = min(end, imp[ctr["idx"]][0]) if ctr["idx"] < len(imp) else end   # :167-171
                    if clipped <= pos:                                         # :173-178
                        continue
                    span = (pos, clipped, (note_id, params))
                    break
            ctr["pos"] = span[1]                                               # :88
            if span[2] is not None:                                            # :90-100
                changed = True if self.note is None else span[2][0] != self.note[0]   # :96-99: the ids, nothing else
                self.note = span[2]
                return (span[0], span[1], span[2][1], changed)
        return None

    def spans(self, start, end, impulses):
        """the Trigger.next loop over counter(Span(start, end), impulses): -> [(s, e, params, note_id_changed)]"""
        ctr = self.counter(start, end, impulses)
        return list(iter(lambda: self.next(ctr), None))


# ---- a span-table stage's table
def table(players_spans, max_spans):
    """the stage's table from each player's inner sub-spans [(s, e, (freq, note_on), changed)]: rows at max_spans and beyond are
    dropped and counted"""
    N = len(players_spans)
    tb = {"count": np.zeros(N, np.uint32), "start": np.zeros((max_spans, N), np.uint32), "end": np.zeros((max_spans, N), np.uint32),
          "nic": np.zeros((max_spans, N), np.uint8), "freq": np.zeros((max_spans, N), f32), "note_on": np.zeros((max_spans, N), np.uint32)}
    dropped = 0
    for p, spans in enumerate(players_spans):
        tb["count"][p] = min(len(spans), max_spans)
        dropped += max(0, len(spans) - max_spans)
        for k, (s, e, (freq, on), changed) in enumerate(spans[:max_spans]):
            tb["start"][k, p], tb["end"][k, p], tb["nic"][k, p], tb["freq"][k, p], tb["note_on"][k, p] = s, e, changed, freq, on
    return tb, dropped


def live_rows(ref):
    """[K][N] bools: the rows below each player's count"""
    return np.arange(ref["start"].shape[0])[:, None] < ref["count"][None, :]


def same_table(got, ref, names=("start", "end", "nic", "note_on", "freq")):
    """counts equal, and every row below a player's count equal on bits in the arrays `names`; -> None or what differs first"""
    if not np.array_equal(got["count"], ref["count"]):
        return ("count", np.argwhere(got["count"] != ref["count"])[:4].tolist())
    K, live = ref["start"].shape[0], live_rows(ref)
    for name in names:
        a, b = got[name][:K], ref[name]
        if b.dtype == f32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a[live], b[live]):
            return (name, np.argwhere((a != b) & live)[:4].tolist())
    return None


# ---- a voice's state as uint32 words.  STATE: [(object or None, field, kind, ...)] in the struct's order, kind "f" = f32
def float_words(STATE):
    return np.array([k == "f" for _, _, k in STATE])


def state_words(voices):
    return np.array([v.words() for v in voices], np.uint32)


def struct_state(STATE, st):
    """a modules.*.state() array -> [V][words] uint32 in STATE's order"""
    return np.stack([np.ascontiguousarray(st[s[1]] if s[0] is None else st[s[0]][s[1]]).view(np.uint32) for s in STATE], axis=1)


def same_words(float_mask, a, b):
    """two [V][words] arrays: integers equal, floats (float_mask) bit for bit except that any NaN equals any NaN"""
    fw = np.asarray(float_mask)
    fa, fb = np.ascontiguousarray(a[:, fw]).view(f32), np.ascontiguousarray(b[:, fw]).view(f32)
    na, nb = np.isnan(fa), np.isnan(fb)
    return bool(np.array_equal(a[:, ~fw], b[:, ~fw]) and np.array_equal(na, nb) and np.array_equal(fa.view(np.uint32)[~na], fb.view(np.uint32)[~nb]))
