"""The curve-voice tests' data, shared by tests/test_curve_player_host.py, tests/test_gpu_curve_player.py and
tests/test_gpu_curve_voice_player.py; holds no tests.  The five-effect kit, per-voice sub-span tables whose effect and rel_freq
differ per sub-span, and the two base images.  Everything is compared on bits."""
import numpy as np

from tests import curve_player_reference as cr
from tests.laser_cases import FIXED, LINEAR, MAX_SPANS, ROWS, SMOOTHSTEP, SPAN, SR, base_image, ms, same_bits  # noqa: F401
from tests.span_reference import walk

N_EFFECTS = 5


def kit_effects():
    """Five effects (modulator, carrier, volume); every volume curve is empty -- the voice never reads it.  Node times of a few
    frames at 48 kHz -- 48 and 144 -- so that nodes fall inside, at the start of and at the end of the tables' sub-spans.
    0: smoothstep / smoothstep; 1: a linear carrier; 2: an EMPTY modulator curve (the phase is 0 + sin(t_m) of a phase that
    never moves); 3: single nodes; 4: a carrier of 40 nodes two frames apart: more span nodes than one sub-span's table holds."""
    short = [(0.0, 800.0), (ms(48), 300.0), (ms(144), 120.0)]
    dense = [(ms(2 * i), 200.0 + 150.0 * float((i * 7) % 5)) for i in range(40)]
    none = ([], SMOOTHSTEP)
    return [
        ((short, SMOOTHSTEP), ([(0.0, 600.0), (ms(48), 900.0), (ms(144), 200.0)], SMOOTHSTEP), none),
        ((short, SMOOTHSTEP), ([(0.0, 500.0), (ms(47), 1500.0), (ms(145), 100.0)], LINEAR), none),
        (([], SMOOTHSTEP), (short, SMOOTHSTEP), none),
        (([(ms(10), 440.0)], SMOOTHSTEP), ([(0.0, 220.0)], LINEAR), none),
        (([(0.0, 300.0), (ms(100), 50.0)], LINEAR), (dense, SMOOTHSTEP), none),
    ]


def long_kit_effects():
    """two effects whose curves last about 700 frames at 48 kHz: a note crosses at least two edges of 256-frame buffers"""
    return [(([(0.0, 110.0), (ms(300), 55.0), (ms(700), 220.0)], SMOOTHSTEP),
             ([(0.0, 440.0), (ms(120), 880.0), (ms(256), 110.0), (ms(400), 660.0), (ms(512), 330.0), (ms(700), 20.0)], SMOOTHSTEP), ([], SMOOTHSTEP)),
            (([(0.0, 200.0), (ms(690), 20.0)], LINEAR), ([(0.0, 300.0), (ms(255), 900.0), (ms(705), 100.0)], LINEAR), ([], SMOOTHSTEP))]


def tables(V, seed, second=False):
    """One buffer's table: count [V], start / end / nic [K][V] and the two fields' [K][V] arrays.  Voices 0-4 hold the FIXED
    patterns of the laser's tables (adjacent, empty, out of order, both edges, none), the rest are seeded.  Effect of sub-span
    k, voice v: (v + k) % 6 -- 5 is the kit's count, out of range.  `second`: the buffer after that one -- every first sub-span
    has note_id_changed clear and effect (v + 4) % 6, which differs from the effect of every sub-span the first buffer's table
    gave voice v last."""
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
    kk, vv = np.meshgrid(np.arange(K), np.arange(V), indexing="ij")
    effect = ((vv + kk + (4 if second else 0)) % 6).astype(np.uint32)
    if second:
        nic[0, :] = 0
    else:
        nic[0, 0] = 1; nic[2, 0] = 0                                 # voice 0: its third sub-span switches the effect, note_id_changed clear
    return {"count": count, "start": start, "end": end, "nic": nic.astype(np.uint8),
            "rel_freq": rng.uniform(0.5, 2.0, (K, V)).astype(np.float32), "effect": effect}


def span_values(tb, names=cr.FIELDS):
    """`values` of modules.CurveVoice.span_table for the named fields"""
    return {n: ((None, tb[n]) if n == "effect" else (tb[n], None)) for n in names}


def walked(tb, V):
    """[(v, k, start, end, nic, effect)] of the sub-spans the span paints' walk reaches"""
    S, E = SPAN
    out = []
    for v in range(V):
        for k, s, e in walk(tb, v, S, E):
            out.append((v, k, s, e, int(tb["nic"][k, v]), int(tb["effect"][k, v])))
    return out
