"""The detuned-voice tests' data, shared by tests/test_detuned_host.py, tests/test_gpu_detuned.py and
tests/test_gpu_detuned_player.py; holds no tests.  Per-voice sub-span tables whose freq, note_on and mode differ per sub-span,
the short test patch, the planted warble values and the hostile ones.  Everything is compared on bits; any NaN equals any NaN
(tests/hostile_cases.py same_f32: by position, not by payload)."""
import numpy as np

from tests import detuned_reference as dr

SR = 48000.0
ROWS, SPAN = 256, (3, 250)
MAX_SPANS = 4
FIRST_SEED = 1000
ms = lambda frames: frames / SR                    # a duration of `frames` frames at 48 kHz

# attack, decay and release of a few dozen frames, so that all four envelope stages fall inside sub-spans; a warble filter fast
# enough to move within a sub-span
TEST_PATCH = dr.Patch(warble_hz=400.0, attack=ms(15), decay=ms(25), release=ms(40), res=0.3)
DEFAULT_PATCH = dr.Patch()

FIXED = [[(3, 51), (51, 51), (51, 195), (195, 250)],                 # adjacent, an empty one between, both edges
         [(10, 120), (100, 170), (180, 200)],                        # the second starts before the first ends: the list ends there
         [(3, 3), (250, 250)],                                       # empty at either edge: the prologues still run
         [(20, 21), (21, 250)],
         []]                                                         # no sub-span at all

# Unplanted, |w| stays below 0.125 (40 buffers x 8 seeds on the oracle): pow never leaves its fractional arm.  noise_filter.l
# planted through set_state reaches the integer loop, the reciprocal arm, denormal results (2^-149.6 x 220), underflow to 0
# and overflow to inf (after which the voice is NaN from its second frame on); each value in mode 0 and in mode 1.
PLANTED = [0.2, -0.2, 1.3, -1.3, 7.6, -7.6, 31.9, 32.1, -37.4, 40.0, -160.0]
HOSTILE_FREQ = [np.nan, np.inf, -np.inf, 0.0, -0.0, -220.0, 1e-40, 3e38, 6000.0, 24000.0, 1e9]
HOSTILE_SR = [0.0, -48000.0, np.nan, np.inf, 1e-40]
NAN_CAP = 0.25                                     # of the compared samples (hostile freq: the oracle alone gives 0.08; sample_rate: 0.18)


def tables(V, seed, note_on_first=True):
    """One buffer's table: count [V], start / end / nic [K][V] and the three fields' [K][V] arrays.  Voices 0-4 hold the FIXED
    patterns, the rest are seeded.  note_on: mostly set; cleared in about a third of the later sub-spans (a release inside the
    buffer).  mode: 0-3 (only bit 0 reaches the voice)."""
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
    return {"count": count, "start": start, "end": end, "nic": nic.astype(np.uint8),
            "freq": rng.uniform(110.0, 880.0, (K, V)).astype(np.float32), "note_on": note_on,
            "mode": rng.integers(0, 4, (K, V)).astype(np.uint32)}


def one_span_tables(V, seed):
    """every voice: one sub-span, the whole SPAN"""
    tb = tables(V, seed)
    S, E = SPAN
    return {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
            "nic": tb["nic"][:1], "freq": tb["freq"][:1], "note_on": tb["note_on"][:1], "mode": tb["mode"][:1]}


def base_image(V, seed):
    """random, with -0.0 planted: in every frame from 200 on of the odd voices and in one frame in eight elsewhere"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.0, 1.0, (V, ROWS)).astype(np.float32)
    img[rng.random((V, ROWS)) < 0.125] = -0.0
    img[1::2, 200:] = -0.0
    return img


def span_values(tb, names=dr.FIELDS):
    """`values` of modules.Detuned.span_table for the named fields"""
    return {n: ((tb[n], None) if n == "freq" else (None, tb[n])) for n in names}


def gpu_patch(p):
    from zang_amd import modules as mod
    return mod.Detuned.Patch(**p.__dict__)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def nan_share(*arrays):
    return sum(int(np.isnan(a).sum()) for a in arrays) / max(1, sum(a.size for a in arrays))
