"""The shapes and streams of the controlled phase-modulation voice's tests; holds no tests.  Everything is small: images of 100
rows, buffers of 1, 7 and 96 frames, at most seven rows per stream and voice.  SR and the patch are chosen so that a control's
glide takes 24 frames (0.006 s at 4 kHz; the reference's 4,800 frames would never reach paintFlat here) -- it both arrives inside
a 96-frame buffer and straddles a buffer edge -- and the envelope's stages take 8, 12 and 16 frames.

streams(V, F, seed) makes the three tables of one buffer.  Rows are drawn per voice and per stream from sorted random cut points
(so empty rows, adjacent rows and gaps all occur) and voice v gets one feature by (v + seed) % 8:
  0  the ratio stream has no row at all            1  the ratio's first row starts after the buffer's first frame
  2  notes and multiplier both end a row at one frame, and begin the next there
  3  all three streams do                          4  every stream has an empty row in the middle
  5  the notes' second row starts before the first one ends: it ends the notes' list, the controls go on
  6, 7  nothing special
Rows at and above a voice's count hold values no walk may read."""
import numpy as np

from tests import mouse_reference as mr

f32 = np.float32
SR = 4000.0
ROWS = 100
SPANS = {1: (5, 6), 7: (2, 9), 96: (2, 98)}        # the buffer of F frames inside the image
VOICES = [1, 63, 64, 65, 130]
K = 7
PATCH = mr.Patch(ctl_curve=mr.CURVE_LINEAR, ctl_glide=0.006, attack=0.002, decay=0.003, release=0.004, sustain_volume=0.25)
SCALES = {True: (4.0, 2.0), False: (880.0, 2.0)}   # relative -> (ratio scale, multiplier scale)   example_mouse.zig:161-164, :185
POISON = 0xdead0001


def rows_in(rng, lo, hi, n, start_at_lo=False, end_at_hi=False):
    """n rows between lo and hi from 2n sorted cut points"""
    pts = np.sort(rng.integers(lo, hi + 1, 2 * n))
    if n and start_at_lo:
        pts[0] = lo
    if n and end_at_hi:
        pts[-1] = hi
    return [(int(pts[2 * k]), int(pts[2 * k + 1])) for k in range(n)]


def voice_rows(rng, S, E, feature):
    """-> the (start, end) rows of the three streams (notes, ratio, multiplier) of one voice"""
    out = [rows_in(rng, S, E, int(rng.integers(0, 7))) for _ in range(3)]
    if feature == 0:
        out[mr.RATIO] = []
    elif feature == 1:
        out[mr.RATIO] = rows_in(rng, min(S + 1 + int(rng.integers(0, 3)), E), E, int(rng.integers(1, 4)), start_at_lo=True)
    elif feature in (2, 3):
        c = int(rng.integers(S + 1, E + 1))
        for s in ((mr.NOTES, mr.MULT) if feature == 2 else (mr.NOTES, mr.RATIO, mr.MULT)):
            out[s] = (rows_in(rng, S, c, int(rng.integers(1, 4)), end_at_hi=True) + rows_in(rng, c, E, int(rng.integers(1, 4)), start_at_lo=True))
    elif feature == 4:
        for s in range(3):
            c = int(rng.integers(S, E + 1))
            out[s] = rows_in(rng, S, c, int(rng.integers(0, 3))) + [(c, c)] + rows_in(rng, c, E, int(rng.integers(0, 3)))
    elif feature == 5:
        m = S + max(1, (E - S) // 2)
        out[mr.NOTES] = [(S, m), (S, m)] + rows_in(rng, m, E, int(rng.integers(0, 3)))
    return out


def table(V, value_name):
    return {"count": np.zeros(V, np.uint32), "start": np.full((K, V), POISON, np.uint32), "end": np.full((K, V), POISON, np.uint32),
            "nic": np.ones((K, V), np.uint8), value_name: np.full((K, V), np.nan, f32), "note_on": np.ones((K, V), np.uint32)}


def streams(V, F, seed):
    """-> [notes, ratio, multiplier]: table dicts (count [V]; start, end, nic, freq or value, note_on [K][V])"""
    rng = np.random.default_rng(seed)
    S, E = SPANS[F]
    tbs = [table(V, "freq"), table(V, "value"), table(V, "value")]
    for v in range(V):
        rows = voice_rows(rng, S, E, (v + seed) % 8)
        for s, tb in enumerate(tbs):
            assert len(rows[s]) <= K
            tb["count"][v] = len(rows[s])
            for k, (a, b) in enumerate(rows[s]):
                tb["start"][k, v], tb["end"][k, v] = a, b
                on = rng.random() < (0.6 if s == mr.NOTES else 0.85)
                tb["note_on"][k, v] = int(on)
                tb["nic"][k, v] = int(on and rng.random() < 0.7)
                if s == mr.NOTES:
                    tb["freq"][k, v] = f32(rng.uniform(40.0, 480.0))
                else:
                    tb["value"][k, v] = f32(rng.uniform(0.0, 1.0))
    return tbs


def uniform_controls(V, F, seed, n=3):
    """the two controls with the SAME row boundaries for every voice (values, note_on and nic per voice): what a composition of
    plain Portamento paints can follow.  -> (ratio, multiplier) tables"""
    rng = np.random.default_rng(seed)
    S, E = SPANS[F]
    out = []
    for _ in range(2):
        tb = table(V, "value")
        rows = rows_in(rng, S, E, n)
        tb["count"][:] = len(rows)
        for k, (a, b) in enumerate(rows):
            tb["start"][k], tb["end"][k] = a, b
            tb["note_on"][k] = rng.random(V) < 0.85
            tb["nic"][k] = (tb["note_on"][k] != 0) & (rng.random(V) < 0.7)
            tb["value"][k] = rng.uniform(0.0, 1.0, V).astype(f32)
        out.append(tb)
    return out


def full_rows(V, F, value_name, value, note_on, nic):
    """one row over the whole buffer for every voice"""
    S, E = SPANS[F]
    tb = table(V, value_name)
    tb["count"][:] = 1
    tb["start"][0], tb["end"][0], tb["nic"][0], tb["note_on"][0] = S, E, int(nic), int(note_on)
    tb[value_name][0] = value
    return tb


def held_note(V, buffer):
    """THE stream on which the carried temp shows: a note pressed at the start of buffer 0 and held across the edge into buffer 1,
    both controls held at a constant.  In relative mode buffer 1's modulator frequency is s + r * freq with s = buffer 0's envelope
    at the same buffer index: with the image the output differs from the output without it."""
    nic = buffer == 0
    return [full_rows(V, 96, "freq", f32(220.0), True, nic), full_rows(V, 96, "value", f32(0.5), True, nic),
            full_rows(V, 96, "value", f32(0.75), True, nic)]


def base_image(V, seed, minus_zero=True):
    img = np.random.default_rng(seed).uniform(-1.0, 1.0, (V, ROWS)).astype(f32)
    if minus_zero:
        img[:, ::5] = -0.0
    return img
