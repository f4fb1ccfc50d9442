"""The builtin modules' span paints (zh_<module>_paint_spans) as test cases: per module its span fields and their random values,
the plain params that hold where a field has no span array, the oracle's per-sub-span paint and the state to compare; random
per-voice sub-span tables; and _run, which paints buffers with both and compares them bit for bit.  Shared by
tests/test_gpu_module_spans.py and tools/module_spans_bench.py."""
import ctypes as C

import numpy as np

from tests import util

SR = 48000.0
F = 1024
K = 3
# cob images (the plain paint's zang.buffer): the kind -> the span field it stands in for, and the range of its values
IMAGES = {"freq_img": ("freq", 20.0, 7000.0), "phase_img": ("phase", -1.0, 1.0), "cut_img": ("cutoff", 0.0, 1.0), "res_img": ("res", 0.0, 1.0)}


def _tables(V, nbuf, seed, geo=None):
    """Per buffer, per voice: 0-3 ascending sub-spans (s, e, note_id_changed) -- adjacent, gapped, empty, touching either edge.
    Voice 0: the carry-over pattern of tests/test_gpu_spans.py::_random_tables (trigger_test.zig:77-115).  geo (a
    paint_cases.Geometry): the sub-spans are drawn inside geo.span instead of [0, F), voice 0's pattern scaled to it."""
    rng = np.random.default_rng(seed)
    lo, hi = (0, F) if geo is None else geo.span
    at = lambda f: lo + (hi - lo) * f // F                       # frame f of [0, F) inside [lo, hi)
    bufs = []
    for _ in range(nbuf):
        per_voice = []
        for _ in range(V):
            k = int(rng.integers(0, K + 1))
            cuts = np.sort(rng.integers(lo, hi + 1, size=2 * k))
            spans, prev = [], lo
            for j in range(k):
                s, e = int(cuts[2 * j]), int(cuts[2 * j + 1])
                r = rng.random()
                if r < 0.25:
                    s = prev                                     # adjacent to the previous one / at the buffer start
                elif r < 0.35:
                    e = s                                        # empty
                if j == k - 1 and rng.random() < 0.3:
                    e = hi                                       # ends with the buffer
                s = max(s, prev); e = max(e, s)
                spans.append((s, e, bool(rng.random() < 0.5)))
                prev = e
            per_voice.append(spans)
        bufs.append(per_voice)
    bufs[0][0] = [(lo, at(200), True), (at(200), hi, True)]
    if nbuf > 1:
        bufs[1][0] = [(lo, at(500), False), (at(500), at(600), True), (at(600), hi, False)]
    if nbuf > 2:
        bufs[2][0] = [(lo, hi, False)]
    return bufs


def _arrays(per_voice):
    V = len(per_voice)
    count = np.array([len(x) for x in per_voice], np.uint32)
    start = np.zeros((K, V), np.uint32); end = np.zeros((K, V), np.uint32); nic = np.zeros((K, V), np.uint8)
    for v, spans in enumerate(per_voice):
        for k, (s, e, n) in enumerate(spans):
            start[k, v], end[k, v], nic[k, v] = s, e, n
    return count, start, end, nic


# ------------------------------------------------------------------ the modules: span fields, defaults, oracle
# A field: (name, gen) with gen(rng, shape) -> (f array or None, u array or None).  `dflt` gives the value a field has without a
# span array: {name: (f [V] or None, u scalar or [V] or None)}.
def _f(lo, hi, special=()):
    def gen(rng, shape):
        a = rng.uniform(lo, hi, shape).astype(np.float32)
        for i, x in enumerate(special):
            a.flat[i::7 + i] = x
        return a, None
    return gen


def _u(n):
    return lambda rng, shape: (None, rng.integers(0, n, shape).astype(np.uint32))


def _curve(rng, shape):
    return rng.uniform(0.0005, 0.03, shape).astype(np.float32), rng.integers(0, 4, shape).astype(np.uint32)


class _Case:
    stateful = True
    inputs = False
    first_seed = 0
    dev = staticmethod(util.dev)        # a per-voice default array on the device (_run with a geometry: Geometry.per_voice)

    def value(self, name, k, v):
        f, u = self.arr.get(name, (None, None))
        df, du = self.dflt[name]
        fv = f[k, v] if f is not None else (df[v] if df is not None else None)
        uv = u[k, v] if u is not None else (du[v] if isinstance(du, np.ndarray) else du)
        return fv, uv


class SineCase(_Case):
    name = "sineosc"
    fields = [("freq", _f(20.0, 3000.0)), ("phase", _f(-1.0, 1.0))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.SineOsc(V, ctx)

    def params(self, m, d, extra):
        from zang_amd import zang
        freq = zang.buffer(extra["freq_img"]) if "freq_img" in extra else zang.constant(self.dev(d["freq"][0]))
        phase = zang.buffer(extra["phase_img"]) if "phase_img" in extra else zang.constant(self.dev(d["phase"][0]))
        return m.Params(SR, freq, phase)

    def oracle_init(self, o, L):
        s = o.SineOsc(); L.zo_sineosc_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        fb, pb = ex.get("freq_img_host"), ex.get("phase_img_host")
        freq = o.buffer(fb[v]) if fb is not None else o.constant(self.value("freq", k, v)[0])
        phase = o.buffer(pb[v]) if pb is not None else o.constant(self.value("phase", k, v)[0])
        L.zo_sineosc_paint(C.byref(st), s, e, o.fptr(row), SR, freq, phase)

    def state(self, m, sts):
        return [(m.state()["t"].astype(np.float32), np.array([x.t for x in sts], np.float32))]


class PulseCase(SineCase):
    name = "pulseosc"
    fields = [("freq", _f(20.0, 3000.0, special=(-5.0, 7000.0))), ("color", _f(0.0, 1.0))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.PulseOsc(V, ctx)

    def params(self, m, d, extra):
        from zang_amd import zang
        freq = zang.buffer(extra["freq_img"]) if "freq_img" in extra else zang.constant(self.dev(d["freq"][0]))
        return m.Params(SR, freq, self.dev(d["color"][0]))

    def oracle_init(self, o, L):
        s = o.PulseOsc(); L.zo_pulseosc_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        fb = ex.get("freq_img_host")
        freq = o.buffer(fb[v]) if fb is not None else o.constant(self.value("freq", k, v)[0])
        L.zo_pulseosc_paint(C.byref(st), s, e, o.fptr(row), SR, freq, self.value("color", k, v)[0])

    def state(self, m, sts):
        return [(m.state()["cnt"].astype(np.uint32), np.array([x.cnt for x in sts], np.uint32))]


class TriSawCase(PulseCase):
    name = "trisawosc"
    fields = [("freq", _f(20.0, 3000.0, special=(-5.0, 7000.0))), ("color", _f(0.0, 1.0, special=(0.0,)))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.TriSawOsc(V, ctx)

    def oracle_init(self, o, L):
        s = o.TriSawOsc(); L.zo_trisawosc_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        fb = ex.get("freq_img_host")
        freq = o.buffer(fb[v]) if fb is not None else o.constant(self.value("freq", k, v)[0])
        L.zo_trisawosc_paint(C.byref(st), s, e, o.fptr(row), SR, freq, self.value("color", k, v)[0])

    def state(self, m, sts):
        g = m.state()
        return [(g["cnt"].astype(np.uint32), np.array([x.cnt for x in sts], np.uint32)),
                (g["t"].astype(np.float32), np.array([x.t for x in sts], np.float32))]


class NoiseCase(_Case):
    name = "noise"
    fields = [("color", _u(2))]
    first_seed = 77

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.Noise(V, ctx, first_seed=self.first_seed)

    def params(self, m, d, extra):
        return m.Params(int(d["color"][1]))

    def oracle_init(self, o, L, v=0):
        s = o.Noise(); L.zo_noise_init(C.byref(s), self.first_seed + v); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        L.zo_noise_paint(C.byref(st), s, e, o.fptr(row), int(self.value("color", k, v)[1]))

    def state(self, m, sts):
        return [(m.state()["r"].astype(np.uint64), np.array([list(x.r) for x in sts], np.uint64))]


class EnvCase(_Case):
    name = "envelope"
    fields = [("attack", _curve), ("decay", _curve), ("release", _curve), ("sustain_volume", _f(0.2, 1.0, special=(1.0,))),
              ("note_on", _u(2))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.Envelope(V, ctx)

    def params(self, m, d, extra):
        from zang_amd import abi
        from zang_amd.runtime import as_f32
        curves = []
        for n in ("attack", "decay", "release"):
            dur = self.dev(d[n][0])
            c = abi.Curve(int(d[n][1]), 0, as_f32(dur))
            c._keep = dur                                        # (the struct holds the pointer: keep the tensor behind it alive)
            curves.append(c)
        on = d["note_on"][1]
        return m.Params(SR, *curves, self.dev(d["sustain_volume"][0]), self.dev(on.astype(np.uint8)))

    def oracle_init(self, o, L):
        s = o.Envelope(); L.zo_envelope_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        cv = [o.curve(int(self.value(n, k, v)[1]), self.value(n, k, v)[0]) for n in ("attack", "decay", "release")]
        p = o.EnvelopeParams(SR, cv[0], cv[1], cv[2], self.value("sustain_volume", k, v)[0], int(self.value("note_on", k, v)[1] != 0))
        L.zo_envelope_paint(C.byref(st), s, e, o.fptr(row), int(nic), C.byref(p))

    def state(self, m, sts):
        g = m.state()
        return [(g["state"].astype(np.uint32), np.array([x.state for x in sts], np.uint32)),
                (g["t"].astype(np.float32), np.array([x.painter.t for x in sts], np.float32)),
                (g["last_value"].astype(np.float32), np.array([x.painter.last_value for x in sts], np.float32)),
                (g["start"].astype(np.float32), np.array([x.painter.start for x in sts], np.float32))]


class GateCase(_Case):
    name = "gate"
    stateful = False
    fields = [("note_on", _u(2))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.Gate(V, ctx)

    def params(self, m, d, extra):
        return m.Params(self.dev(d["note_on"][1].astype(np.uint8)))

    def oracle_init(self, o, L):
        return None

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        L.zo_gate_paint(s, e, o.fptr(row), int(self.value("note_on", k, v)[1] != 0))

    def state(self, m, sts):
        return []


class FilterCase(_Case):
    name = "filter"
    inputs = True
    fields = [("type", _u(6)), ("cutoff", _f(0.0, 1.1)), ("res", _f(0.0, 1.0))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.Filter(V, ctx)

    def params(self, m, d, extra):
        from zang_amd import zang
        cut = zang.buffer(extra["cut_img"]) if "cut_img" in extra else zang.constant(self.dev(d["cutoff"][0]))
        res = zang.buffer(extra["res_img"]) if "res_img" in extra else zang.constant(self.dev(d["res"][0]))
        return m.Params(extra["input"], int(d["type"][1]), cut, res)

    def oracle_init(self, o, L):
        s = o.Filter(); L.zo_filter_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        cb, rb = ex.get("cut_img_host"), ex.get("res_img_host")
        cut = o.buffer(cb[v]) if cb is not None else o.constant(self.value("cutoff", k, v)[0])
        res = o.buffer(rb[v]) if rb is not None else o.constant(self.value("res", k, v)[0])
        L.zo_filter_paint(C.byref(st), s, e, o.fptr(row), o.fptr(ex["input_host"][v]), int(self.value("type", k, v)[1]), cut, res)

    def state(self, m, sts):
        g = m.state()
        return [(g["l"].astype(np.float32), np.array([x.l for x in sts], np.float32)),
                (g["b"].astype(np.float32), np.array([x.b for x in sts], np.float32))]


class SamplerCase(_Case):
    name = "sampler"
    fields = [("sample_rate", _f(8000.0, 96000.0, special=(44100.0, -44100.0, -22050.0, 44100.5))), ("loop", _u(2))]
    fmt = 1
    channels, in_rate = 2, 44100

    def make(self, ctx, V):
        from zang_amd import modules as mod
        rng = np.random.default_rng(60 + self.fmt)
        self.data = rng.integers(0, 256, 700 * self.channels * (self.fmt + 1), dtype=np.uint8)
        self.ddev = util.dev(self.data)
        return mod.Sampler(V, ctx)

    def params(self, m, d, extra):
        smp = m.Sample(self.channels, self.in_rate, self.fmt, self.ddev)
        return m.Params(self.dev(d["sample_rate"][0]), smp, self.channels - 1, bool(d["loop"][1]))

    def oracle_init(self, o, L):
        s = o.Sampler(); L.zo_sampler_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        p = o.SamplerParams(float(self.value("sample_rate", k, v)[0]), self.channels, self.in_rate, self.fmt,
                            self.data.ctypes.data_as(C.POINTER(C.c_uint8)), self.data.size, self.channels - 1,
                            int(self.value("loop", k, v)[1] != 0))
        L.zo_sampler_paint(C.byref(st), s, e, o.fptr(row), int(nic), C.byref(p))

    def state(self, m, sts):
        return [(m.state()["t"].astype(np.float32), np.array([x.t for x in sts], np.float32))]


class DecimatorCase(_Case):
    name = "decimator"
    inputs = True
    fields = [("fake_sample_rate", _f(100.0, 40000.0, special=(48000.0, 60000.0, -5.0, 0.0)))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.Decimator(V, ctx)

    def params(self, m, d, extra):
        return m.Params(SR, extra["input"], self.dev(d["fake_sample_rate"][0]))

    def oracle_init(self, o, L):
        s = o.Decimator(); L.zo_decimator_init(C.byref(s)); return s

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        L.zo_decimator_paint(C.byref(st), s, e, o.fptr(row), SR, o.fptr(ex["input_host"][v]), self.value("fake_sample_rate", k, v)[0])

    def state(self, m, sts):
        g = m.state()
        return [(g["dval"].astype(np.float32), np.array([x.dval for x in sts], np.float32)),
                (g["dcount"].astype(np.float32), np.array([x.dcount for x in sts], np.float32))]


class DistortionCase(_Case):
    name = "distortion"
    stateful = False
    inputs = True
    fields = [("type", _u(2)), ("ingain", _f(0.0, 1.0)), ("outgain", _f(0.0, 1.0)), ("offset", _f(-0.5, 0.5))]

    def make(self, ctx, V):
        from zang_amd import modules as mod
        return mod.Distortion(V, ctx)

    def params(self, m, d, extra):
        return m.Params(extra["input"], int(d["type"][1]), self.dev(d["ingain"][0]), self.dev(d["outgain"][0]), self.dev(d["offset"][0]))

    def oracle_init(self, o, L):
        return None

    def oracle_paint(self, o, L, st, v, s, e, row, nic, k, ex):
        L.zo_distortion_paint(s, e, o.fptr(row), o.fptr(ex["input_host"][v]), int(self.value("type", k, v)[1]),
                              self.value("ingain", k, v)[0], self.value("outgain", k, v)[0], self.value("offset", k, v)[0])

    def state(self, m, sts):
        return []


CASES = {c.name: c for c in (SineCase, PulseCase, TriSawCase, NoiseCase, EnvCase, GateCase, FilterCase, SamplerCase, DecimatorCase,
                             DistortionCase)}
UINT_DEFAULT_PER_VOICE = {"note_on"}     # zh_bool fields: a per-voice default; every other `u` field's default is one value


def _defaults(case, rng, V):
    d = {}
    for name, gen in case.fields:
        f, u = gen(rng, (V,))
        if u is not None and name not in UINT_DEFAULT_PER_VOICE:
            u = u[0]
        d[name] = (f, u)
    return d


def _span_kernels(ctx, case, zeroed):
    """the kernels of the last paint: k_<module>_spans -- behind the one kernel that zeroes the span where a ZERO_FIRST paint reads
    an image that overlaps its output (zeroed: may it; a bool, or "must")"""
    form = ctx.last_form()
    assert form[-1:] == ["k_%s_spans" % case.name] and form[:-1] in ([], ["k_elementwise"]), form
    assert zeroed or len(form) == 1, form
    assert zeroed != "must" or len(form) == 2, form


def _field_arrays(case, rng, V, mode, imaged):
    case.arr = {}
    for name, gen in case.fields:
        if mode == "none" or name in imaged:
            continue
        if mode == "mix" and rng.random() < 0.5:
            continue
        case.arr[name] = gen(rng, (K, V))


def _run(ctx, oracle, case, V, seed, mode="arrays", images=(), nbuf=4, geo=None):
    """Paint nbuf buffers of random per-voice sub-span tables with the spans form and with the oracle, voice by voice; compare
    the images and the state after every buffer.  Buffers alternate ADD (onto random content) and ZERO_FIRST (onto garbage).
    mode: "arrays" = every span field varies per sub-span, "none" = no span arrays (span_params NULL: the per-voice / broadcast
    params hold), "mix" = some fields with arrays, the rest from the params.  images: kinds of IMAGES given as cob buffers.
    geo (a paint_cases.Geometry): the images are its views (the output role "out", the module input "in", cob images "ctl"), the
    per-voice default arrays its slices, the painted span and the tables' range geo.span, and its canaries are checked after every
    buffer.  -> the oracle's images, one per buffer."""
    import torch
    from zang_amd import zang
    rng = np.random.default_rng(seed)
    L = oracle.lib()
    m = case.make(ctx, V)
    sts = [case.oracle_init(oracle, L, v) if isinstance(case, NoiseCase) else case.oracle_init(oracle, L) for v in range(V)]
    rows = F if geo is None else geo.frames
    lo, hi = (0, F) if geo is None else geo.span
    image = util.to_image if geo is None else (lambda h, role: geo.image(role, content=util.to_image(h)))
    bufs = _tables(V, nbuf, seed + 1, geo)
    if geo is not None:
        case.dev = geo.per_voice
    case.dflt = _defaults(case, rng, V)
    ex, extra, refs = {}, {}, []
    for kind in images:
        h = rng.uniform(IMAGES[kind][1], IMAGES[kind][2], (V, rows)).astype(np.float32)
        ex[kind + "_host"] = h; extra[kind] = util.to_image(h) if geo is None else image(h, "ctl")
    imaged = {IMAGES[kind][0] for kind in images}
    for b in range(nbuf):
        count, start, end, nic = _arrays(bufs[b])
        _field_arrays(case, rng, V, mode, imaged)
        if case.inputs:
            ex["input_host"] = util.rng_buffers(seed + 10 + b, V, rows)
            extra["input"] = util.to_image(ex["input_host"]) if geo is None else image(ex["input_host"], "in")
        zf = b % 2 == 1
        base = util.rng_buffers(seed + 20 + b, V, rows)
        ref = base.copy()
        if zf:
            ref[:, lo:hi] = 0.0
        for v in range(V):
            for k, (s, e, n) in enumerate(bufs[b][v]):
                case.oracle_paint(oracle, L, sts[v], v, s, e, ref[v], n, k, ex)
        out = util.to_image(base) if geo is None else image(base, "out")
        table = m.span_table(count, start, end, nic, None if mode == "none" else case.arr)
        m.paint_spans(zang.Span(lo, hi), [out], None, case.params(m, case.dflt, extra), table, zero_first=zf)
        ctx.sync()
        # (views of ONE allocation: their extents overlap, so a ZERO_FIRST paint that reads an image zeroes its span first)
        _span_kernels(ctx, case, zf and geo is not None and geo.name == "shared_allocation" and bool(images or case.inputs))
        util.assert_bitexact(util.from_image(out), ref, f"{case.name} V={V} buffer {b} zf={zf}")
        for gpu, cpu in case.state(m, sts):
            util.assert_bitexact(gpu, cpu, f"{case.name} V={V} state after buffer {b}")
        if geo is not None:
            geo.check_canaries(f"{case.name} buffer {b}")
            geo.release([out] + ([extra["input"]] if case.inputs else []))
        refs.append(ref)
    m.close()
    torch.cuda.synchronize()
    return refs


# which image of a module can BE its output (_run_in_place): the kind of IMAGES, or "input"
IN_PLACE = [("sineosc", "freq_img"), ("sineosc", "phase_img"), ("pulseosc", "freq_img"), ("trisawosc", "freq_img"), ("filter", "input"),
            ("filter", "cut_img"), ("filter", "res_img"), ("decimator", "input"), ("distortion", "input")]
# ... and what it holds at first: a frequency of some hundreds of Hz (the +-1 of a frame's own add moves the phase), else the kind's range
IN_PLACE_RANGE = {"freq_img": (200.0, 900.0), "input": (-1.0, 1.0)}


def _run_in_place(ctx, oracle, case, V, seed, geo, which, mode="mix"):
    """The span paint with the image `which` BEING the output (one tensor), as paint_cases.Shared.zf_seq: ADD onto the image's own
    content, ZERO_FIRST, ADD from the state those left -- against the oracle given one row as output and as that image (it zeroes
    the row's span before the ZERO_FIRST step), bit for bit, images, states and canaries.  A second oracle run takes a COPY of the
    row (as it is before each paint) as the image.  -> (the oracle's images, the copy run's), one per paint."""
    import torch
    from zang_amd import zang
    assert geo.in_place
    rng = np.random.default_rng(seed)
    L = oracle.lib()
    m = case.make(ctx, V)
    sts, sts2 = ([case.oracle_init(oracle, L) for v in range(V)] for _ in range(2))
    rows = geo.frames
    lo, hi = geo.span
    zf_seq = (False, True, False)
    bufs = _tables(V, len(zf_seq), seed + 1, geo)
    case.dev = geo.per_voice
    case.dflt = _defaults(case, rng, V)
    r = IN_PLACE_RANGE.get(which, IMAGES.get(which, (None, None, None))[1:])
    ref = rng.uniform(r[0], r[1], (V, rows)).astype(np.float32)
    ref2 = ref.copy()
    out = geo.image("out", content=util.to_image(ref))
    key = "input_host" if which == "input" else which + "_host"
    ex, extra = {key: ref}, {("input" if which == "input" else which): out}
    ex2 = {}
    if case.inputs and which != "input":
        ex["input_host"] = util.rng_buffers(seed + 10, V, rows)
        extra["input"] = geo.image("in", content=util.to_image(ex["input_host"]))
        ex2["input_host"] = ex["input_host"]
    imaged = {IMAGES[which][0]} if which in IMAGES else set()
    refs, refs2 = [], []
    for b, zf in enumerate(zf_seq):
        count, start, end, nic = _arrays(bufs[b])
        _field_arrays(case, rng, V, mode, imaged)
        ex2[key] = ref2.copy()
        if zf:
            ref[:, lo:hi] = 0.0; ref2[:, lo:hi] = 0.0
        for v in range(V):
            for k, (s, e, n) in enumerate(bufs[b][v]):
                case.oracle_paint(oracle, L, sts[v], v, s, e, ref[v], n, k, ex)
                case.oracle_paint(oracle, L, sts2[v], v, s, e, ref2[v], n, k, ex2)
        table = m.span_table(count, start, end, nic, case.arr)
        m.paint_spans(zang.Span(lo, hi), [out], None, case.params(m, case.dflt, extra), table, zero_first=zf)
        ctx.sync()
        _span_kernels(ctx, case, "must" if zf else False)
        util.assert_bitexact(util.from_image(out), ref, f"{case.name} V={V}, {which} is the output, paint {b} zf={zf}")
        for gpu, cpu in case.state(m, sts):
            util.assert_bitexact(gpu, cpu, f"{case.name} V={V}, {which} is the output, state after paint {b}")
        geo.check_canaries(f"{case.name} in place, paint {b}")
        refs.append(ref.copy()); refs2.append(ref2.copy())
    m.close()
    torch.cuda.synchronize()
    return refs, refs2
