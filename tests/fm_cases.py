"""The corpus of the FM tests, shared by the CPU coverage test (tests/test_fm_reference.py) and the GPU tests: 130 voices in 26
instruments of 5 (two full waves and a 2-lane tail; group boundaries inside a wave), 1,024 frames, painted as the chain
(0,200) (200,777) (777,1024) (0,1024) with note_on / note_id_changed changing between the paints.  The reference (tests/fm_reference.py)
is computed once per process and shared; nothing here needs a GPU."""
import functools

import numpy as np

from tests import fm_reference as fr

V, GROUP, F, SR = 130, 5, 1024, 48000.0
NI = V // GROUP
CHAIN = ((0, 200), (200, 777), (777, 1024), (0, 1024))
SEED = 20261018
ZERO_HZ_VOICE, SILENT_VOICE = 3, 7


@functools.lru_cache(maxsize=None)
def patches():
    """26 patches: 0 the default, 1 the default with algorithm 0, the rest random inside num_values with the axes the coverage
    test names forced in by index -- every waveform pair, feedback, freq_mul 0 and 10-15, every volume and sustain bit, attack /
    decay / release at 0 and 15 (15 = 2 ms = 96 frames: such voices run through every envelope stage inside the chain)."""
    rng = np.random.default_rng(SEED)
    out = []
    for j in range(NI):
        p = [int(rng.integers(0, n)) for n in fr.NUM_VALUES]
        p[fr.MOD_WAVEFORM], p[fr.CAR_WAVEFORM] = j % 4, (j // 4) % 4
        p[fr.MOD_FEEDBACK] = j % 8
        p[fr.ALGORITHM] = (j // 2) % 2
        p[fr.MOD_FREQ_MUL] = (0, 10, 11, 12, 13, 14, 15, 1, 2, 3)[j % 10]
        p[fr.CAR_FREQ_MUL] = (1, 2, 0, 15, 14, 13, 12, 11, 10, 4)[j % 10]
        p[fr.MOD_VOLUME], p[fr.CAR_VOLUME] = 1 << (j % 6), (1 << ((j + 3) % 6)) if j % 5 else 0
        p[fr.MOD_SUSTAIN], p[fr.CAR_SUSTAIN] = 1 << (j % 4), 1 << ((j + 1) % 4)
        # envelope times: fast everywhere (15) except where an axis wants 0 or a release that is still running 577 frames later (12)
        p[fr.MOD_ATTACK], p[fr.CAR_ATTACK] = (0 if j % 9 == 4 else 15), (0 if j % 9 == 5 else 15)
        p[fr.MOD_DECAY], p[fr.CAR_DECAY] = (0 if j % 7 == 3 else 15), (0 if j % 7 == 4 else 15)
        p[fr.MOD_RELEASE], p[fr.CAR_RELEASE] = (15, 12, 0, 15)[j % 4], (12, 15, 15, 0)[j % 4]
        p[fr.MOD_TREMOLO], p[fr.CAR_TREMOLO] = j % 2, (j // 2) % 2
        p[fr.MOD_VIBRATO], p[fr.CAR_VIBRATO] = (j // 3) % 2, (j // 5) % 2
        p[fr.TREMOLO_DEPTH], p[fr.VIBRATO_DEPTH] = (j // 4) % 2, (j // 6) % 2
        out.append(tuple(p))
    out[0] = fr.DEFAULT_PATCH
    out[1] = tuple(0 if k == fr.ALGORITHM else x for k, x in enumerate(fr.DEFAULT_PATCH))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def inputs():
    """-> dict: freq [V], trem / vib [NI][F] (arbitrary signals in [-1, 1]: the LFOs are inputs here), live [V][F] (what the output
    holds before the first paint), and per paint of the chain note_on [V], nic [V]"""
    rng = np.random.default_rng(SEED + 1)
    freq = rng.uniform(50.0, 2000.0, V).astype(np.float32)
    freq[ZERO_HZ_VOICE] = 0.0
    trem = rng.uniform(-1.0, 1.0, (NI, F)).astype(np.float32)
    vib = rng.uniform(-1.0, 1.0, (NI, F)).astype(np.float32)
    live = rng.uniform(-1.0, 1.0, (V, F)).astype(np.float32)
    u = rng.random((len(CHAIN), V))
    on = np.zeros((len(CHAIN), V), bool)
    nic = np.zeros((len(CHAIN), V), bool)
    on[0], nic[0] = u[0] < 0.9, True                                 # most notes begin with the chain
    on[1] = on[0] & (u[1] < 0.5)                                     # half of them are released at frame 200 ...
    on[2] = u[2] < 0.7                                               # ... and most come back at 777, as new notes where they were off
    nic[2] = on[2] & ~on[1]
    on[3] = u[3] < 0.5
    nic[3] = on[3] & (~on[2] | (u[3] < 0.25))                       # (note_on without a new id while releasing is the reference's assert)
    on[:, SILENT_VOICE] = False
    nic[:, SILENT_VOICE] = False
    return {"freq": freq, "trem": trem, "vib": vib, "live": live, "on": on, "nic": nic}


@functools.lru_cache(maxsize=None)
def reference():
    """The chain through the helper -> dict: per paint m, c [V][n], add_m [V], state (fm_reference.STATE_DTYPE [V][2]) after it;
    `classes` [operator][|p| class] and `stages` over the whole chain; `release_at` [paint][V]: an envelope in RELEASE when the paint starts"""
    from oracle import pyoracle as po
    x = inputs()
    ref = fr.FMRef(V, GROUP, patches())
    paints, release_at = [], []
    for k, (s, e) in enumerate(CHAIN):
        st = ref.state()
        release_at.append((st["env_state"] == po.ENV_RELEASE).any(axis=1))
        m, c, add_m = ref.paint(s, e, x["nic"][k], SR, x["trem"], x["vib"], x["freq"], x["on"][k])
        paints.append({"m": m, "c": c, "add_m": add_m, "state": ref.state()})
    return {"paints": paints, "classes": ref.classes.copy(), "stages": set(ref.stages), "release_at": release_at}


def expected_images(base):
    """the unsplit chain added onto base [V][F] -> the image after every paint"""
    out, img = [], base.copy()
    for k, (s, e) in enumerate(CHAIN):
        p = reference()["paints"][k]
        fr.add_into(img, np.arange(V), s, e, p["m"], p["c"], p["add_m"])
        out.append(img.copy())
    return out


# ---- span tables: three consecutive buffers, 0-3 sub-spans per voice from six shapes (so that the helper's frame-sequential loop
# runs once per distinct sub-span, not once per voice)
SPAN_SHAPES = ((),                                                   # an empty voice
               ((0, 1024),),
               ((0, 300), (300, 700)),                               # two that touch
               ((100, 101), (500, 1024)),                            # a single frame; one that ends with the buffer
               ((0, 200), (200, 777), (777, 1024)),                  # three that touch, the last to the buffer's end
               ((37, 500), (600, 901)))
SPAN_BUFFERS = 3


@functools.lru_cache(maxsize=None)
def span_tables():
    """-> per buffer {count [V], start / end / freq / note_on / note_id_changed [3][V]}"""
    rng = np.random.default_rng(SEED + 2)
    out = []
    prev_on = np.zeros(V, bool)          # a note that is on again after an off is a new note (without a new id: the reference's assert)
    for b in range(SPAN_BUFFERS):
        tb = {"count": np.zeros(V, np.uint32), "start": np.zeros((3, V), np.uint32), "end": np.zeros((3, V), np.uint32),
              "freq": np.zeros((3, V), np.float32), "note_on": np.zeros((3, V), np.uint8), "note_id_changed": np.zeros((3, V), np.uint8)}
        for v in range(V):
            shape = SPAN_SHAPES[(v + 2 * b) % len(SPAN_SHAPES)]
            tb["count"][v] = len(shape)
            for k, (s, e) in enumerate(shape):
                tb["start"][k, v], tb["end"][k, v] = s, e
                tb["freq"][k, v] = 0.0 if v == ZERO_HZ_VOICE else rng.uniform(50.0, 2000.0)
                on = rng.random() < 0.65
                tb["note_on"][k, v] = on
                tb["note_id_changed"][k, v] = on and (not prev_on[v] or rng.random() < 0.7)
                prev_on[v] = on
        out.append(tb)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def span_reference():
    """the three buffers through the helper's Trigger loop, state carried -> per buffer (m, c, painted, add_m, state)"""
    x = inputs()
    ref = fr.FMRef(V, GROUP, patches())
    out = []
    for tb in span_tables():
        m, c, painted, add_m = ref.paint_spans(0, F, SR, x["trem"], x["vib"], tb)
        out.append((m, c, painted, add_m, ref.state()))
    return tuple(out)
