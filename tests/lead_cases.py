"""The lead-voice tests' data, shared by tests/test_lead_host.py, tests/test_gpu_lead.py and tests/test_gpu_lead_players.py; holds
no tests.  Per-voice sub-span tables whose freq and note_on differ per sub-span (the shapes of tests/detuned_cases.py), the short
test patches and the hostile values.  Everything is compared on bits; any NaN equals any NaN (tests/hostile_cases.py same_f32: by
position, not by payload)."""
from dataclasses import dataclass

import numpy as np

from tests import lead_reference as lr
from tests.span_reference import walk

SR = 48000.0
ROWS, SPAN = 256, (3, 250)
MAX_SPANS = 4
HOSTILE_FROM = 200                                 # hostile values enter in frames >= 200 only: at most 50 of the 247 compared
ms = lambda frames: frames / SR                    # a duration of `frames` frames at 48 kHz

FIXED = [[(3, 51), (51, 51), (51, 195), (195, 250)],                 # adjacent, an empty one between, both edges
         [(10, 120), (100, 170), (180, 200)],                        # the second starts before the first ends: the list ends there
         [(3, 3), (250, 250)],                                       # empty at either edge: prologue and epilogue still run
         [(20, 21), (21, 250)],
         []]                                                         # no sub-span at all

HOSTILE_FREQ = [np.nan, np.inf, -np.inf, 0.0, -0.0, -220.0, 1e-40, 3e38, 6000.0, 24000.0, 1e9]
HOSTILE_SR = [0.0, -48000.0, np.nan, np.inf, 1e-40]
# 50 of 247 frames (0.20) is the most a hostile value can turn NaN, since it acts from frame 200 on; the cap leaves room above it
NAN_CAP = 0.25


@dataclass
class Kind:
    """one of the two voices: its names on both sides"""
    name: str
    voice: type                                    # lr.PortaVoice / lr.VibratoVoice
    paint: object                                  # lr.porta_paint / lr.vibrato_paint
    test_patch: object
    default_patch: object

    def module(self):
        from zang_amd import modules as mod
        return mod.Porta if self.name == "porta" else mod.Vibrato

    def gpu_patch(self, p):
        return self.module().Patch(**p.__dict__)

    def voices(self, oracle, V):
        return [self.voice(oracle) for _ in range(V)]


# attack, decay, release and glide of 15-40 frames: every envelope stage, a finished and an unfinished glide fall inside sub-spans;
# a vibrato fast and deep enough to move the pulse's frequency within a sub-span
PORTA = Kind("porta", lr.PortaVoice, lr.porta_paint,
             lr.PortaPatch(glide=ms(30), attack=ms(15), decay=ms(25), release=ms(40)), lr.PortaPatch())
VIBRATO = Kind("vibrato", lr.VibratoVoice, lr.vibrato_paint, lr.VibratoPatch(vib_hz=400.0, depth=0.3, color=0.3), lr.VibratoPatch())
KINDS = [PORTA, VIBRATO]
KIND_IDS = [k.name for k in KINDS]


def tables(V, seed, note_on_first=True):
    """One buffer's table: count [V], start / end / nic [K][V] and the two fields' [K][V] arrays.  Voices 0-4 hold the FIXED
    patterns, the rest are seeded.  note_on: set in about two thirds of the sub-spans, so that on->on (with note_id_changed set
    and clear), on->off, off->on and off->off all occur."""
    rng = np.random.default_rng(seed)
    K, (S, E) = MAX_SPANS, SPAN
    count = np.zeros(V, np.uint32)
    start, end, nic = (np.zeros((K, V), np.uint32) for _ in range(3))
    for v in range(V):
        if v < len(FIXED):
            spans = FIXED[v]
        else:
            k = int(rng.integers(0, K + 1))
            cuts = np.sort(rng.integers(S, E + 1, 2 * k))
            spans, prev = [], S
            for j in range(k):
                s, e = int(cuts[2 * j]), int(cuts[2 * j + 1])
                r = rng.random()
                if r < 0.25:
                    s = prev
                elif r < 0.35:
                    e = s
                s = max(s, prev); e = max(e, s)
                spans.append((s, e)); prev = e
        count[v] = len(spans)
        for k, (s, e) in enumerate(spans):
            start[k, v], end[k, v] = s, e
    nic[:] = rng.integers(0, 2, (K, V))
    note_on = (rng.random((K, V)) < 0.67).astype(np.uint32)
    if note_on_first:
        note_on[0, :] = 1; nic[0, :] = 1
    # voice 0 alone (V = 1) sees all four pairs and both kinds of on->on over a first and a later buffer
    if note_on_first:
        note_on[:, 0] = (1, 1, 1, 0); nic[:, 0] = (1, 0, 1, 1)
    else:
        note_on[:, 0] = (0, 1, 1, 1); nic[:, 0] = (1, 1, 0, 1)
    return {"count": count, "start": start, "end": end, "nic": nic.astype(np.uint8),
            "freq": rng.uniform(110.0, 880.0, (K, V)).astype(np.float32), "note_on": note_on}


def pairs(tbs):
    """the (prev_note_on, note_on, note_id_changed) triples that the sub-spans reached in these consecutive buffers hold, from a
    voice that starts with prev_note_on clear (the walk's contract decides which are reached)"""
    seen = set()
    V = len(tbs[0]["count"])
    prev = np.zeros(V, bool)
    for tb in tbs:
        S, E = SPAN
        for v in range(V):
            for k, _, _ in walk(tb, v, S, E):
                on = bool(tb["note_on"][k, v])
                seen.add((bool(prev[v]), on, bool(tb["nic"][k, v])))
                prev[v] = on
    return seen


ALL_PAIRS = {(False, False), (False, True), (True, False), (True, True)}


def covers_every_pair(tbs):
    seen = pairs(tbs)
    return {(p, n) for p, n, _ in seen} == ALL_PAIRS and (True, True, True) in seen and (True, True, False) in seen


def one_span_tables(V, seed):
    """every voice: one sub-span, the whole SPAN"""
    tb = tables(V, seed)
    S, E = SPAN
    return {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
            "nic": tb["nic"][:1], "freq": tb["freq"][:1], "note_on": tb["note_on"][:1]}


def hostile_freq_tables(seed=31337):
    """Every value of HOSTILE_FREQ in the LAST sub-span of a voice, which starts at HOSTILE_FROM or later; its two earlier
    sub-spans are ordinary.  Hostile voice i once alone in its wave (voice 64 * i) and once among the other hostile ones (voices
    64 * n ...), with note_on set and clear; everything else ordinary."""
    n = len(HOSTILE_FREQ)
    V = 64 * n + 64
    tb = tables(V, seed)
    for i, x in enumerate(HOSTILE_FREQ):
        for j, v in enumerate((64 * i, 64 * n + i)):
            s = HOSTILE_FROM + 3 * i
            tb["count"][v] = 3
            tb["start"][:3, v], tb["end"][:3, v] = (3, 80, s), (80, s, 250)
            tb["freq"][:3, v] = (220.0, 440.0, x)
            tb["note_on"][:3, v] = (1, 1, 1 - j)
    return V, tb


def base_image(V, seed):
    """random, with -0.0 planted: in every frame from 200 on of the odd voices and in one frame in eight elsewhere"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.0, 1.0, (V, ROWS)).astype(np.float32)
    img[rng.random((V, ROWS)) < 0.125] = -0.0
    img[1::2, 200:] = -0.0
    return img


def span_values(tb, names=lr.FIELDS):
    """`values` of modules.Porta / Vibrato .span_table for the named fields"""
    return {n: ((tb[n], None) if n == "freq" else (None, tb[n])) for n in names}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def nan_share(*arrays):
    return sum(int(np.isnan(a).sum()) for a in arrays) / max(1, sum(a.size for a in arrays))


def worst_row_nan_share(*arrays):
    """the largest NaN share of any voice's compared frames [SPAN) over the given [V][ROWS] images"""
    S, E = SPAN
    return max(float(np.isnan(a[:, S:E]).mean(axis=1).max()) for a in arrays)
