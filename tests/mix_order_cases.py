"""Inputs shared by tests/test_mix_order_reference.py (CPU) and tests/test_gpu_mix_order.py: the voice counts, the spans, the random
images and the planted columns of the tree mixdown with their hand-derived sums."""
import numpy as np

F32 = np.float32
EPS = float(np.finfo(np.float32).eps)

# quad tails, wave and tile edges, 17 tiles (per = 2) and 34 tiles (per = 3: the second pass's segment split)
TREE_VS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028, 2049, 16385, 33793]
TREE_ROWS = 80
# under, at and over the 8-frame first-pass group and the 64-frame second-pass block; (5, 5) is empty
TREE_SPANS = [(0, 1), (3, 10), (3, 11), (5, 12), (0, 64), (1, 66), (7, 80), (5, 5)]
PLANTED_VS = [1025, 2049]

FUSED_ROWS = 128
# whole and partial 32-frame chunks, partial 8-frame partial-row groups, a span straddling a chunk edge, an empty one
FUSED_SPANS = [(0, 32), (5, 37), (5, 78), (31, 33), (9, 9)]


def random_image(V, rows, seed=9):
    """[V][rows] uniform in (-1, 1)"""
    return np.random.default_rng(seed + 1000003 * V).uniform(-1.0, 1.0, (V, rows)).astype(F32)


def random_row(rows, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, rows).astype(F32)


def integer_image(V, rows, seed=5):
    """integer-valued, |x| <= 100: every partial sum of up to 167,772 voices stays below 2^24 and every add is exact"""
    return np.random.default_rng(seed + V).integers(-100, 101, (V, rows)).astype(F32)


# ---- planted cancellation columns: B = 1e8 (f32 spacing 8 there, so B + 1 = B and 1 - B = -B), 1.0 and -B, everything else +0.0.
# One frame per placement; `want` is derived by hand from the order basics.hip:168-173 states, for zero_first (dst = 0.0f + tot).
B = 1e8
PLANTED = [
    # --- one quad: ((x0 + x1) + x2) + x3
    ({0: B, 1: 1.0, 2: -B}, 0.0),          # ((B + 1) + -B) + 0 = (B + -B) + 0 = 0
    ({0: B, 1: -B, 2: 1.0}, 1.0),          # ((B + -B) + 1) + 0 = 1
    ({1: 1.0, 2: B, 3: -B}, 0.0),          # ((0 + 1) + B) + -B = B + -B = 0
    # --- two lanes of wave 0: the quads first, then the butterfly; the steps 32 .. 2 meet zeros, step 1 adds lane 1 to lane 0
    ({0: B, 4: 1.0, 5: -B}, 0.0),          # lane 0 = B; lane 1 = (1 + -B) = -B; B + -B = 0
    ({0: B, 1: -B, 4: 1.0}, 1.0),          # lane 0 = B + -B = 0; lane 1 = 1; 0 + 1 = 1
    # --- three lanes: step 2 pairs lane 0 with 2 and lane 1 with 3, step 1 then pairs the results
    ({0: B, 4: 1.0, 8: -B}, 1.0),          # step 2: lane 0 = B + -B = 0, lane 1 = 1 + 0; step 1: 0 + 1 = 1  (sequential order gives 0)
    ({0: B, 4: -B, 8: 1.0}, 0.0),          # step 2: lane 0 = B + 1 = B, lane 1 = -B; step 1: B + -B = 0     (sequential order gives 1)
    # --- lanes 0 and 32: the butterfly's first step
    ({0: B, 4: 1.0, 128: -B}, 1.0),        # step 32: lane 0 = B + -B = 0, lane 1 = 1; ... step 1: 0 + 1 = 1
    # --- two waves (voices 256 .. 511 are wave 1): ((w0 + w1) + w2) + w3
    ({0: B, 4: 1.0, 256: -B}, 0.0),        # w0 = B + 1 = B, w1 = -B; (B + -B) + 0 + 0 = 0
    ({0: B, 4: -B, 256: 1.0}, 1.0),        # w0 = 0, w1 = 1
    ({0: B, 256: 1.0, 512: -B}, 0.0),      # (B + 1) + -B = 0
    ({0: B, 256: -B, 512: 1.0}, 1.0),      # (B + -B) + 1 = 1
    ({256: 1.0, 512: B, 768: -B}, 0.0),    # ((0 + 1) + B) + -B = 0
    # --- two tiles (voice 1024 opens tile 1; 2 or 3 tiles: per = 1, one tile per segment): tot = seg0 + seg1 + ...
    ({0: B, 1: 1.0, 1024: -B}, 0.0),       # tile 0 = B + 1 = B, tile 1 = 0 + -B (a cut quad at V = 1025, a whole one at 2049); B + -B = 0
    ({0: B, 1: -B, 1024: 1.0}, 1.0),       # tile 0 = 0, tile 1 = 1
    ({0: 1.0, 512: B, 1024: -B}, 0.0),     # tile 0 = (1 + 0) + B = B; B + -B = 0
]


def planted_image(V):
    """([V][len(PLANTED)] image, expected sums) -- every planted voice index is below 1025"""
    img = np.zeros((V, len(PLANTED)), F32)
    want = np.zeros(len(PLANTED), F32)
    for f, (cells, w) in enumerate(PLANTED):
        for v, x in cells.items():
            img[v, f] = x
        want[f] = w
    return img, want


SUBNORMAL = F32(1e-40)


def special_image(V, rows=24, seed=77):
    """A random image with subnormal voices in frames 2 and 3 (every voice 1e-40 in frame 2: quads, lanes and waves add
    subnormals to subnormals, and an add that flushed them would leave 0; frame 3: subnormals among ordinary voices), one NaN at (frame 5, voice V - 2), +Inf at (frame 9, voice 1) and -Inf
    at (frame 17, voice V // 2).  Returns (image [V][rows], the frames whose sum is NaN / +Inf / -Inf: compared by class)."""
    img = random_image(V, rows, seed)
    img[:, 2] = SUBNORMAL
    img[::3, 3] = SUBNORMAL
    img[V - 2, 5] = np.nan
    img[1, 9] = np.inf
    img[V // 2, 17] = -np.inf
    return img, {5: "nan", 9: "+inf", 17: "-inf"}


def float_class(x):
    return "nan" if np.isnan(x) else "+inf" if x == np.inf else "-inf" if x == -np.inf else "finite"


# ---- the fused mixdown's voices: gains with both zeros, 1.0, a negative one and ordinary pans in every wave (from 16 voices up)
def fused_gains(u2):
    V = len(u2)
    gl = (0.5 + 0.5 * (2.0 * u2.astype(np.float64) - 1.0)).astype(F32)
    gr = (F32(1.0) - gl).astype(F32)
    i = np.arange(V)
    gl[i % 16 == 1] = 0.0;  gr[i % 16 == 1] = 1.0
    gl[i % 16 == 2] = -0.0; gr[i % 16 == 2] = 0.0
    gl[i % 16 == 5] = 1.0;  gr[i % 16 == 5] = -0.0
    gl[i % 16 == 9] = -0.75; gr[i % 16 == 9] = 1.75
    return gl, gr


def silence_some(freq):
    """a few voices of every wave silenced (begin() silences a frequency above sr / 8 or below 0): +0.0 columns"""
    freq = freq.copy()
    freq[3::64] = 7000.0
    freq[40::64] = -1.0
    return freq
