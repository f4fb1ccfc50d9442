"""The sample kit's test data, shared by tests/test_sample_kit_host.py, tests/test_gpu_sample_kit.py and tests/test_cpp_sample_kit.py:
the seven-sample kit, per-voice sub-span tables whose sample / channel / rate / loop differ per sub-span, and the yardstick --
zo_sampler_paint (oracle/zang_oracle.c, Sampler.zig:23-136 restated) called once per voice and sub-span with that sub-span's
sample descriptor, on host copies of the same bytes.  Everything is compared on bits."""
import ctypes as C

import numpy as np

from tests.span_reference import value, walk  # noqa: F401  (value: for the tests)

ROWS, SPAN = 128, (5, 101)
MAX_SPANS = 4
RATES = [44100.0, 44100.5, 22050.0, -44100.0, -22050.0, 48000.0]
T_SPECIAL = [0.0, -5.5, 1e9, 2.0 ** 31]


def kit_samples():
    """[(num_channels, sample_rate, format, bytes as a uint8 array)]: every format, an empty sample, a one-frame sample, stray
    bytes after the last whole frame, and an s24 sample with stray bytes LAST, at the blob's end."""
    rng = np.random.default_rng(20261018)
    spec = [(1, 44100, 0, 37 * 1), (2, 44100, 1, 50 * 2 * 2), (1, 22050, 2, 41 * 3 + 2), (3, 48000, 3, 23 * 3 * 4), (1, 44100, 1, 0),
            (1, 44100, 1, 1 * 2), (2, 44100, 2, 29 * 2 * 3 + 5)]
    return [(nch, rate, fmt, rng.integers(0, 256, n, dtype=np.uint8)) for nch, rate, fmt, n in spec]


def tables(V, seed, second=False):
    """One buffer's table: count [V], start / end / nic [K][V], and the four fields' [K][V] arrays.  Voices 0-3 hold fixed
    patterns (adjacent and empty sub-spans, one out of order, both span edges); the rest are seeded.  Sample index of sub-span k,
    voice v: (v + k) % 8 -- index 7 is out of range -- and channel (v + 2k) % 4.  `second`: the buffer after that one -- every first
    sub-span has note_id_changed clear and sample (v + 5) % 8, which no sub-span of the first buffer's voice v had last."""
    rng = np.random.default_rng(seed)
    K, (S, E) = MAX_SPANS, SPAN
    count = np.zeros(V, np.uint32)
    start, end, nic = (np.zeros((K, V), np.uint32) for _ in range(3))
    fixed = [[(S, 30), (30, 30), (30, 60), (60, E)],                 # adjacent, an empty one between, both edges
             [(10, 50), (40, 70), (80, 90)],                         # the second starts before the first ends: the list ends there
             [(S, S), (E, E)],                                       # empty at either edge: the prologues still run
             [(20, 21), (21, 100)]]
    for v in range(V):
        if v < len(fixed):
            spans = fixed[v]
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
    sample = ((vv + kk + (5 if second else 0)) % 8).astype(np.uint32)
    channel = ((vv + 2 * kk) % 4).astype(np.uint32)
    if second:
        nic[0, :] = 0
    rate = rng.uniform(8000.0, 96000.0, (K, V)).astype(np.float32)
    pick = rng.integers(0, len(RATES) + 1, (K, V))
    for i, r in enumerate(RATES):
        rate[pick == i] = r
    loop = rng.integers(0, 2, (K, V)).astype(np.uint32)
    return {"count": count, "start": start, "end": end, "nic": nic.astype(np.uint8),
            "sample_rate": rate, "loop": loop, "sample": sample, "channel": channel}


def start_t(V, seed):
    t = np.random.default_rng(seed).uniform(0.0, 60.0, V).astype(np.float32)
    n = min(V, len(T_SPECIAL))
    t[:n] = T_SPECIAL[:n]
    return t


def oracle_params(o, samples, sample, channel, rate, loop):
    """zo_sampler_params of kit entry `sample` (None when there is no such entry: the paint is a no-op)"""
    if sample >= len(samples):
        return None
    nch, in_rate, fmt, data = samples[sample]
    return o.SamplerParams(float(rate), nch, in_rate, fmt, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size, int(channel), int(bool(loop)))


def reference(o, samples, tb, t, img, zero_first, span=SPAN, dflt=None):
    """What the span paint must leave: img [V][rows] and t [V], painted in place.  The walk is the span paints' contract."""
    L = o.lib()
    S, E = span
    V = len(tb["count"])
    if zero_first:
        img[:, S:E] = 0.0
    for v in range(V):
        st = o.Sampler(); st.t = float(t[v])
        for k, s, e in walk(tb, v, S, E):
            p = oracle_params(o, samples, int(value(tb, dflt, "sample", k, v)), value(tb, dflt, "channel", k, v),
                              value(tb, dflt, "sample_rate", k, v), value(tb, dflt, "loop", k, v))
            if p is not None:
                L.zo_sampler_paint(C.byref(st), s, e, o.fptr(img[v]), int(tb["nic"][k, v]), C.byref(p))
        t[v] = st.t
    return img, t


def run_lane_harness(exe, tmp, samples, tb, t, img, zero_first, span=SPAN):
    """the same through tests/cpp/sample_kit_lane_host -> (img, t)"""
    import os
    import subprocess
    V, rows = img.shape
    K = tb["start"].shape[0]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(samples), V, K, rows, span[0], span[1], int(zero_first), 0], np.uint32).tobytes())
        for nch, rate, fmt, data in samples:
            f.write(np.array([nch, rate, fmt, data.size], np.uint32).tobytes())
        for _, _, _, data in samples:
            f.write(data.tobytes())
        f.write(np.ascontiguousarray(t, np.float32).tobytes())
        f.write(tb["count"].astype(np.uint32).tobytes())
        for name in ("start", "end", "nic"):
            f.write(np.ascontiguousarray(tb[name]).astype(np.uint32).tobytes())
        f.write(np.ascontiguousarray(tb["sample_rate"], np.float32).tobytes())
        for name in ("loop", "sample", "channel"):
            f.write(np.ascontiguousarray(tb[name]).astype(np.uint32).tobytes())
        f.write(np.ascontiguousarray(img, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(fout, "rb").read()
    assert len(raw) == (V * rows + V) * 4
    return np.frombuffer(raw, np.float32, V * rows).reshape(V, rows).copy(), np.frombuffer(raw, np.float32, V, V * rows * 4).copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
