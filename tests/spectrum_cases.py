"""The spectrum analyser's case table, shared by the CPU harness test and the GPU tests: one 1,024-frame column per case, the
rest of an image uniform random.  Every case is a value the transform or an epilogue treats in its own way."""
import numpy as np

F32 = np.float32
FRAMES = 1024
BIN = 100
NAMES = ["random", "zero", "dc", "nyquist", "impulse_first", "impulse_last", "cosine", "sine", "negative_zero", "denormal", "one_inf",
         "one_nan", "huge", "overflow", "loud"]


def column(name, seed=1):
    t = np.arange(FRAMES)
    if name == "random":
        return np.random.default_rng(seed).uniform(-1.0, 1.0, FRAMES).astype(F32)
    x = np.zeros(FRAMES, F32)
    if name == "dc":
        x[:] = 1.0
    elif name == "nyquist":
        x[:] = np.where(t % 2 == 0, 1.0, -1.0)
    elif name == "impulse_first":
        x[0] = 1.0
    elif name == "impulse_last":
        x[FRAMES - 1] = 1.0
    elif name == "cosine":
        x[:] = np.cos(2 * np.pi * BIN * t / FRAMES)
    elif name == "sine":
        x[:] = np.sin(2 * np.pi * BIN * t / FRAMES)
    elif name == "negative_zero":
        x[:] = -0.0
    elif name == "denormal":
        x[517] = 1e-42
    elif name == "one_inf":
        x[:] = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, FRAMES)
        x[300] = np.inf
    elif name == "one_nan":
        x[:] = np.random.default_rng(seed + 2).uniform(-1.0, 1.0, FRAMES)
        x[700] = np.nan
    elif name == "huge":
        x[:] = 1e30                      # 1,024 of them are 1.024e33: large, still finite
    elif name == "overflow":
        x[:] = 1e36                      # 1,024 of them add up past f32's range inside the transform: inf, then inf * 0
    elif name == "loud":                 # |X| = 1,536 at bins 0 and 100, 1,280 at 300: hslToRgb sees h in (1, 1.23), channel bytes overlap
        x[:] = 1.5 + 3.0 * np.cos(2 * np.pi * BIN * t / FRAMES) + 2.5 * np.cos(2 * np.pi * 300 * t / FRAMES)
    elif name != "zero":
        raise KeyError(name)
    return x


def image(voices, seed=1, frames=FRAMES):
    """[frames][voices]: column v is (the first frames of) case NAMES[v] while there are cases, every other sample uniform random in [-1, 1)"""
    img = np.random.default_rng(1000 * voices + seed).uniform(-1.0, 1.0, (frames, voices)).astype(F32)
    for v, name in enumerate(NAMES[:voices]):
        k = min(frames, FRAMES)
        img[:k, v] = column(name, seed)[:k]
    return img


def case_voice(name):
    return NAMES.index(name)
