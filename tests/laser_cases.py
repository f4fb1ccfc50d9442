"""The laser tests' data, shared by tests/test_laser_host.py, tests/test_gpu_laser.py and tests/test_gpu_laser_player.py; holds
no tests.  The five-effect kit, per-voice sub-span tables whose effect and scalars differ per sub-span, and the runs both sides
make.  Everything is compared on bits."""
import numpy as np

from tests import laser_reference as lr

SR = 48000.0
ROWS, SPAN = 256, (3, 250)
MAX_SPANS = 4
LINEAR, SMOOTHSTEP = 0, 1
ms = lambda frames: frames / SR                    # a node time that lands on `frames` at 48 kHz


def kit_effects():
    """Five effects (modulator, carrier, volume).  Node times of a few milliseconds -- 48 and 144 frames -- so that nodes fall
    inside, at the start of and at the end of the tables' sub-spans.
    0: smoothstep throughout; 1: a linear carrier curve beside smoothstep ones; 2: an EMPTY volume curve (every product is
    +0.0 * c: the add still happens); 3: single nodes; 4: a volume curve of 40 nodes two frames apart (more than 32 span nodes
    inside one sub-span) and a linear modulator curve of 35."""
    short = [(0.0, 800.0), (ms(48), 300.0), (ms(144), 120.0)]
    vol = [(0.0, 0.0), (ms(24), 1.0), (ms(144), 0.0)]
    dense = [(ms(2 * i), float((i * 7) % 5) / 4.0) for i in range(40)]
    dense_m = [(ms(3 * i), 900.0 - 20.0 * i) for i in range(35)]
    return [
        ((short, SMOOTHSTEP), ([(0.0, 600.0), (ms(48), 900.0), (ms(144), 200.0)], SMOOTHSTEP), (vol, SMOOTHSTEP)),
        ((short, SMOOTHSTEP), ([(0.0, 500.0), (ms(47), 1500.0), (ms(145), 100.0)], LINEAR), ([(0.0, 1.0), (ms(144), 0.0)], LINEAR)),
        (([(0.0, 300.0), (ms(100), 50.0)], LINEAR), (short, SMOOTHSTEP), ([], SMOOTHSTEP)),
        (([(ms(10), 440.0)], SMOOTHSTEP), ([(0.0, 220.0)], LINEAR), ([(ms(5), 0.5)], SMOOTHSTEP)),
        ((dense_m, LINEAR), (short, SMOOTHSTEP), (dense, SMOOTHSTEP)),
    ]


def default_kit_effects():
    from zang_amd import sfx
    return [sfx.default_effect()]


FIXED = [[(3, 51), (51, 51), (51, 195), (195, 250)],                 # adjacent, an empty one between, both edges; nodes at 48 / 144 end sub-spans
         [(10, 120), (100, 170), (180, 200)],                        # the second starts before the first ends: the list ends there
         [(3, 3), (250, 250)],                                       # empty at either edge: the prologues still run
         [(20, 21), (21, 250)],
         []]                                                         # no sub-span at all


def tables(V, seed, second=False):
    """One buffer's table: count [V], start / end / nic [K][V] and the five fields' [K][V] arrays.  Voices 0-4 hold the FIXED
    patterns, the rest are seeded.  Effect of sub-span k, voice v: (v + k) % 6 -- 5 is the kit's count, out of range.  `second`:
    the buffer after that one -- every first sub-span has note_id_changed clear and effect (v + 4) % 6, which differs from the
    effect of every sub-span the first buffer's table gave voice v last."""
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
    pick = lambda vals: np.array(vals, np.float32)[rng.integers(0, len(vals), (K, V))]
    return {"count": count, "start": start, "end": end, "nic": nic.astype(np.uint8),
            "freq_mul": rng.uniform(0.85, 1.15, (K, V)).astype(np.float32), "carrier_mul": pick([2.0, 4.0, 0.5, 1.0]),
            "modulator_mul": pick([0.5, 0.125, 9.0]), "modulator_rad": pick([0.5, 1.0, 0.625]), "effect": effect}


def base_image(V, seed):
    """random, with -0.0 planted: in every frame from 200 on of the odd voices (past every effect's last node wherever a
    sub-span began before frame 56), and in one frame in eight elsewhere"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.0, 1.0, (V, ROWS)).astype(np.float32)
    img[rng.random((V, ROWS)) < 0.125] = -0.0
    img[1::2, 200:] = -0.0
    return img


def span_values(tb, names=lr.FIELDS):
    """`values` of modules.Laser.span_table for the named fields"""
    return {n: ((None, tb[n]) if n == "effect" else (tb[n], None)) for n in names}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
