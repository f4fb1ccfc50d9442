"""The per-module oracle drivers of the dispatch tests, over a GEOMETRY: where the images of a paint lie in memory.

Each `case_*` makes carried paints of one module on the GPU, runs the oracle for the sampled voices, and compares image columns
and final states bit for bit.  Everything a case needs from its surroundings comes from a `Geometry`: the number of rows of every
image, the span, the delay length, the images themselves (`image(role)`: a float32 view [frames, V] into a larger backing tensor)
and the per-voice parameter arrays (`per_voice(array)`: a contiguous slice of a longer 1-D tensor).

Every backing tensor is filled with one canary bit pattern (a quiet NaN with a payload), four guard rows above and below the view
and guard floats left and right of it in every row, and is snapshotted as int32 when it is made.  `Geometry.check_canaries()`
asserts after a case that the output backing changed nowhere outside `view columns x span rows`, and that no other image and no
per-voice array changed at all.

The table (offsets in floats from a 16-byte-aligned row start; V = voices):

    name               out               in                 ctl                per-voice arrays
    plain              off 4, V+8        same               same               element 0
    shifted            off 5, V+8        same               same               0      base = 4 mod 16 in every row
    odd_stride         off 4, V+11       same               same               0      rows change alignment class
    mixed_aligned      off 4, V+8        off 8, V+24        off 4, V+40        0      all 16-byte aligned, strides differ
    out_misaligned     off 5, V+8        off 4, V+8         off 4, V+8         0
    in_misaligned      off 4, V+8        off 7, V+12        off 6, V+16        0
    params_shifted     as plain                                                f32 and uint8 at element 1
    shared_allocation  columns [4, 4+V)  [V+12, 2V+12)      [2V+20, 3V+20)     0      ONE backing tensor, stride 3V+24
    in_place           as shifted        IS out (or ctl IS out)                0

(With off 5 and stride V+8 three floats lie right of a row and five left of the next: the eight floats between two rows of a view
are all guards, and all are checked.)

A case paints ONE span twice (ZERO_FIRST, then adding) -- or, with `Geometry(..., spans=[...])`, consecutive spans once each with one
module (the first with ZERO_FIRST, the rest adding onto a zeroed image): `Shared.steps()` walks either plan, for the GPU paints and for
the oracle's.  tests/test_gpu_span_lengths.py uses the second to hand state from one kernel form to the next.  The cases that do not
go through `steps()` (Sampler, PMOscInstrument, Curve, Portamento, the stateless ones) refuse a geometry with `spans`.
"""
import ctypes as C

import numpy as np

SR = 48000.0
CANARY = 0x7fa5c3e1            # a quiet NaN with a payload: no paint computes it
CANARY_BYTE = 0xa5
GUARD_ROWS = 4                 # 4 * stride * 4 bytes is a multiple of 16 for any stride: the alignment classes hold
PV_GUARD = 4                   # guard elements before a per-voice array (16 bytes of f32, and 16 of uint8: see per_voice)

_PLAIN = {"out": (4, 8), "in": (4, 8), "ctl": (4, 8)}
GEOMETRIES = {
    "plain": dict(_PLAIN),
    "shifted": {"out": (5, 8), "in": (5, 8), "ctl": (5, 8)},
    "odd_stride": {"out": (4, 11), "in": (4, 11), "ctl": (4, 11)},
    "mixed_aligned": {"out": (4, 8), "in": (8, 24), "ctl": (4, 40)},
    "out_misaligned": {"out": (5, 8), "in": (4, 8), "ctl": (4, 8)},
    "in_misaligned": {"out": (4, 8), "in": (7, 12), "ctl": (6, 16)},
    "params_shifted": dict(_PLAIN),
    "shared_allocation": None,                       # three column ranges of one backing tensor
    "in_place": {"out": (5, 8), "in": (5, 8), "ctl": (5, 8)},
}


class _Backing:
    def __init__(self, t):
        self.t, self.snap, self.window = t, None, None     # window = (row0, row1, col0, col1) a paint may write, or None
        self.more = []                                     # further windows (Geometry.writable: a voice's second output column)

    def snapshot(self):
        self.snap = self.t.view(_torch().int32).clone()


def _torch():
    import torch
    return torch


class Geometry:
    """Where the images and per-voice arrays of a test lie: see the module's docstring."""

    def __init__(self, name, V, frames=1024, span=None, delay_samples=300, device="cuda", spans=None):
        assert name in GEOMETRIES, name
        self.name, self.V, self.frames, self.device = name, V, frames, device
        # `spans`: consecutive spans a carried case paints one after the other (the first with ZERO_FIRST, the rest adding)
        # instead of painting ONE span twice; `span` is then their hull, the rows a paint may write
        self.spans = None if spans is None else [tuple(sp) for sp in spans]
        if self.spans is not None:
            assert span is None and name != "in_place" and len(self.spans) >= 1
            assert all(a[1] == b[0] for a, b in zip(self.spans, self.spans[1:])), "the spans follow each other"
            span = (self.spans[0][0], self.spans[-1][1])
        self.span = (0, frames) if span is None else tuple(span)
        self.delay_samples = delay_samples
        self.pv_offset = 1 if name == "params_shifted" else 0
        self.in_place = name == "in_place"
        self.images = []                # _Backing of every image tensor (one per image; shared_allocation: one per three)
        self.arrays = []                # _Backing of every per-voice array
        self._shared = []               # shared_allocation: the backings, and which roles of each are handed out
        self._out = None                # shared_allocation: the one output view
        self._last = {}                 # role -> the backing of the view handed out last

    # ---- images
    def _canary(self, shape):
        torch = _torch()
        return torch.full(shape, CANARY, dtype=torch.int32, device=self.device).view(torch.float32)

    def layout(self, role):
        """(offset of the view in its row, row stride), in floats"""
        V = self.V
        if self.name == "shared_allocation":
            return {"out": 4, "in": V + 12, "ctl": 2 * V + 20}[role], 3 * V + 24
        off, pad = GEOMETRIES[self.name][role]
        return off, V + pad

    def image(self, role, content=None, fill=None):
        """A float32 view [frames, V] for `role` in "out" / "in" / "ctl", inside a canary-filled backing tensor.  `content`
        ([frames, V]) or `fill` is written to the view before the backing is snapshotted; an output view is the one window a
        paint may write (its span rows).  shared_allocation: the three roles are column ranges of one tensor (a second request for
        a role opens a second tensor; the output is always the first one's, restored to the canary at every request)."""
        off, stride = self.layout(role)
        rows = self.frames + 2 * GUARD_ROWS
        if self.name == "shared_allocation":
            if role == "out" and self._out is not None:
                b, view = self._out
                view.copy_(self._canary((self.frames, self.V)))
            else:
                slot = next((s for s in self._shared if role not in s[1]), None)
                if slot is None:
                    slot = (_Backing(self._canary((rows, stride))), set())
                    self._shared.append(slot); self.images.append(slot[0])
                slot[1].add(role)
                b = slot[0]
                view = b.t[GUARD_ROWS:GUARD_ROWS + self.frames, off:off + self.V]
                if role == "out":
                    self._out = (b, view)
        else:
            b = _Backing(self._canary((rows, stride)))
            self.images.append(b)
            view = b.t[GUARD_ROWS:GUARD_ROWS + self.frames, off:off + self.V]
        if content is not None:
            view.copy_(content)
        elif fill is not None:
            view.fill_(float(fill))
        if role == "out":
            b.window = (GUARD_ROWS + self.span[0], GUARD_ROWS + self.span[1], off, off + self.V)
            b.more = []
        self._last[role] = b
        b.snapshot()
        return view

    def writable(self, role):
        """The view of `role` handed out last is an output too (a voice's second column, outputs[1]): its span rows may change."""
        off, _ = self.layout(role)
        self._last[role].more.append((GUARD_ROWS + self.span[0], GUARD_ROWS + self.span[1], off, off + self.V))

    def per_voice(self, array):
        """A contiguous 1-D device slice holding `array` (float32 or uint8 / bool) at the geometry's element offset from a
        16-byte-aligned address, guard elements before and after it."""
        torch = _torch()
        a = np.ascontiguousarray(array)
        if a.dtype == np.bool_:
            a = a.view(np.uint8)
        assert a.ndim == 1 and a.dtype in (np.float32, np.uint8), (a.dtype, a.shape)
        lead = PV_GUARD if a.dtype == np.float32 else 16
        n = lead + self.pv_offset + a.size + PV_GUARD
        if a.dtype == np.float32:
            t = self._canary((n,))
        else:
            t = torch.full((n,), CANARY_BYTE, dtype=torch.uint8, device=self.device)
        s = t[lead + self.pv_offset: lead + self.pv_offset + a.size]
        s.copy_(torch.from_numpy(a))
        if a.dtype == np.float32:
            b = _Backing(t)
            b.snapshot()
        else:
            b = _Backing(t)
            b.snap = t.clone()
        self.arrays.append(b)
        return s

    # ---- the canary check
    def release(self, views):
        """Forget the backings of `views` (a case's own outputs, once checked)."""
        ptrs = {v.untyped_storage().data_ptr() for v in views}
        if self.name != "shared_allocation":
            self.images = [b for b in self.images if b.t.untyped_storage().data_ptr() not in ptrs]

    def check_canaries(self, what=""):
        torch = _torch()
        for kind, group in (("image", self.images), ("per-voice array", self.arrays)):
            for k, b in enumerate(group):
                now = b.t.view(torch.int32) if b.t.dtype == torch.float32 else b.t
                diff = now != b.snap
                for r0, r1, c0, c1 in ([] if b.window is None else [b.window]) + b.more:
                    diff[r0:r1, c0:c1] = False
                n = int(diff.sum())
                if n:
                    first = [int(x) for x in torch.nonzero(diff)[0]]
                    where = "outside view x span of an output" if b.window is not None or b.more else "in a tensor no paint may write"
                    raise AssertionError(f"{what} [{self.name}, {self.V} voices]: {n} elements changed {where} ({kind} {k}, "
                                         f"shape {tuple(b.t.shape)}, window {b.window}), first at {first}")


class Target:
    """A case's output and what it paints from: `o` the output view, `src` the image to pass as the input (or control) image,
    `ref` the oracle's [sampled voices][frames] start values, `in_place` whether `src` is `o` (then the oracle passes ref[j] for
    both pointers, as the reference would)."""

    def __init__(self, o, src, ref, cols, in_place):
        self.o, self.src, self.ref, self.cols, self.in_place = o, src, ref, cols, in_place

    def col(self, j):
        return self.ref[j] if self.in_place else self.cols[j]


class Shared:
    """Inputs shared by the cases of one voice count: per-voice params, control / input images, and their sampled columns."""

    def __init__(self, ctx, V, idx, geo=None, alias_ctl=False):
        import torch
        from zang_amd import workloads
        self.geo = geo = Geometry("plain", V) if geo is None else geo
        assert geo.V == V
        F = self.F = geo.frames
        self.s, self.e = geo.span
        self.D = geo.delay_samples
        self.V, self.idx = V, idx
        self.alias_ctl = alias_ctl          # in_place, a case with an input AND a control image: the control image is the output
        # the paints of a carried case: zero_first of each.  in_place: an ADD onto the image's own content first (ZERO_FIRST leaves
        # an in-place paint nothing but zeros to read), then ZERO_FIRST, then an ADD from the state the first two left
        self.zf_seq = (False, True, False) if geo.in_place else (True, False)
        self.freq, self.color, self.u2, self.u3 = workloads.voice_params(5, 0, V)
        self.gf, self.gc = self.pv(self.freq), self.pv(self.color)
        g = torch.Generator(device="cuda"); g.manual_seed(1234 + V)
        wob = 1.0 + 0.25 * torch.rand(F, 1, device="cuda", generator=g)
        self.fbuf = geo.image("ctl", content=self.gf[None, :].expand(F, V) * wob)                                  # a frequency image
        self.ibuf = geo.image("in", content=torch.rand(F, V, device="cuda", generator=g) * 2.0 - 1.0)              # an input signal
        self.cbuf = geo.image("ctl", content=torch.rand(F, V, device="cuda", generator=g) * 0.9 + 0.02)            # cutoffs in (0, 1)
        tidx = torch.from_numpy(idx).cuda()
        self.tidx = tidx
        self.fcol = np.ascontiguousarray(self.fbuf[:, tidx].cpu().numpy().T)
        self.icol = np.ascontiguousarray(self.ibuf[:, tidx].cpu().numpy().T)
        self.ccol = np.ascontiguousarray(self.cbuf[:, tidx].cpu().numpy().T)
        self.pcm = np.random.default_rng(4).integers(-20000, 20000, 9000, dtype=np.int16).view(np.uint8).copy()
        self.gpcm = _dev(self.pcm)
        self.outs = []
        self.forms = {}                     # case name -> kernels its last paint launched

    def span(self):
        from zang_amd import zang
        return zang.Span(self.s, self.e)

    def pv(self, a):
        return self.geo.per_voice(a)

    def cols(self, img):
        return np.ascontiguousarray(img[:, self.tidx].cpu().numpy().T)

    def out(self, fill=None):
        if fill is None and self.geo.spans is not None:
            fill = 0.0                      # consecutive spans: all but the first ADD, onto the zeros the oracle's image starts from
        o = self.geo.image("out", fill=fill)
        self.outs.append(o)
        return o

    def target(self, image=None, cols=None, role="in"):
        """The output of a case that reads `image` (sampled columns `cols`).  in_place: the output starts as a copy of the image
        and IS the image the case paints from."""
        n = len(self.idx)
        if image is not None and self.geo.in_place:
            o = self.geo.image("out", content=image)
            self.outs.append(o)
            return Target(o, o, cols.copy(), cols, True)
        return Target(self.out(), image, np.zeros((n, self.F), np.float32), cols, False)

    def steps(self, zf_seq=None):
        """The carried paints of a case, in order: yields (k, zero_first) with self.s / self.e set to the k-th paint's span.  One
        span (the default): the span painted once per entry of `zf_seq` (self.zf_seq if None).  A geometry with `spans`: one
        paint per span, the first with the first entry of `zf_seq`, the rest adding.  Afterwards self.s / self.e are the hull."""
        seq = self.zf_seq if zf_seq is None else tuple(zf_seq)
        spans = self.geo.spans
        plan = [(self.geo.span, zf) for zf in seq] if spans is None else [(sp, seq[0] if k == 0 else False) for k, sp in enumerate(spans)]
        try:
            for k, ((s, e), zf) in enumerate(plan):
                self.s, self.e = s, e
                yield k, zf
        finally:
            self.s, self.e = self.geo.span

    def pieces(self, zf_seq=None):
        """steps() as a list of (s, e, zero_first): what ref_decimator / ref_filter take as their zf_seq"""
        return [(self.s, self.e, zf) for _, zf in self.steps(zf_seq)]

    def one_span(self):
        assert self.geo.spans is None, "this case paints one span twice: it has no form for consecutive spans"

    def paints(self, paint):
        for k, zf in self.steps():
            paint(k, zf)

    def oracle_zero(self, L, oracle, t, j, zf):
        """what the reference's caller does for ZERO_FIRST: zang.zero(span, out), then the paint"""
        if zf:
            L.zo_zero(self.s, self.e, oracle.fptr(t.ref[j]))

    def finish(self, what=""):
        """after a case's own oracle check: the canaries, then forget the case's outputs"""
        self.geo.check_canaries(what)
        self.geo.release(self.outs)
        self.outs = []


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sample_voices(V, n=48):
    idx = set(range(0, V, max(1, V // n)))
    idx |= {0, 1, 63, 64, 65, 255, 256, V - 1, V - 2, V - 64, V - 65, V // 2 - 1, V // 2}
    return np.array(sorted(i for i in idx if 0 <= i < V), dtype=np.int64)


def _crafted_noise_state(k_frames, seed):
    """A xoshiro256++ state whose k_frames-th draw from now is one of Random.float's multi-draw samples (2^-41 per sample)."""
    from tests.test_gpu_modules import _xoshiro_step_back
    rng = np.random.default_rng(seed)
    return _xoshiro_step_back([0, int(rng.integers(1, 1 << 63)), int(rng.integers(1, 1 << 63)), 1 << 41], k_frames)


def noise_draws(sh, which):
    """Where the crafted multi-draw samples of case_noise (`which` = "noise": three voices) and case_noise_filter ("filter": two)
    fall, as draws counted from the first painted frame -- a function of the painted lengths, asserted from the positions
    themselves:
     - one span of n frames painted twice (draws [0, n) and [n, 2 n)): from n = 1 on one falls inside the first paint and one
       inside the second; from n = 128 on one of the first paint's lies past ceil(n / 2) rounded up to 32 frames -- past the first
       frame range however the span is split in two or more, so that k_noise_fix must repaint the voice -- and from n = 2,048 on
       past frame 1,024.  At 1,024 frames: 77, n - 23, n + n // 2 + 3, and 300, n + 9;
     - consecutive spans: one inside the first, one past the first range of the second, one in the later half of the last."""
    spans = sh.geo.spans
    if spans is not None:
        base = spans[0][0]
        s1, e1 = spans[min(1, len(spans) - 1)]
        sl, el = spans[-1]
        first, mid, late = min(77, (spans[0][1] - base) // 2), s1 - base + (e1 - s1) * 7 // 8, sl - base + (el - sl) * 3 // 4
        assert 0 <= first < max(spans[0][1] - base, 1) and first <= mid <= late < max(el - base, 1), (first, mid, late)
        return (first, mid, late) if which == "noise" else (mid, late)
    n = sh.geo.span[1] - sh.geo.span[0]
    if which == "noise":
        pos = (min(77, n // 2), max(n - 23, n // 2), max(n + min(n // 2 + 3, n - 1), 0))
        in_first, in_second = pos[:2], pos[2:]
    else:
        pos = (min(300, max(n - 21, n // 2)), max(n + min(9, n - 1), 0))
        in_first, in_second = pos[:1], pos[1:]
    if n >= 1:
        assert all(0 <= q < n for q in in_first) and all(n <= q < 2 * n for q in in_second), (n, pos)
    if n >= 128 and which == "noise":
        assert pos[1] >= ((n + 1) // 2 + 31) // 32 * 32, (n, pos)          # past the first of two or more ranges of 32 k frames
    if n >= 2048 and which == "noise":
        assert pos[1] > 1024, (n, pos)
    if n == 1024:
        assert pos == ((77, n - 23, n + n // 2 + 3) if which == "noise" else (300, n + 9)), pos
    return pos


# ---------------------------------------------------------------------------------------------- the cases
# each: case(ctx, oracle, sh) -> None; paints on the GPU, runs the oracle for sh.idx, asserts bit-exact images and states

def _check(sh, ctx, name, out, ref, state_pairs):
    from tests import util
    ctx.sync()
    sh.forms[name] = ctx.last_form()                        # the kernels of the case's last paint (zh_last_form)
    util.assert_bitexact(sh.cols(out)[:, sh.s:sh.e], ref[:, sh.s:sh.e], f"{name} at {sh.V} voices: image columns of sampled voices")
    for what, got, want in state_pairs():
        g = np.asarray(got)
        if g.dtype.kind == "f":
            util.assert_bitexact(g.astype(np.float32), np.asarray(want, dtype=np.float32), f"{name} at {sh.V} voices: state {what}")
        else:                                               # (u64 generator words: never through a float array)
            flat = [int(x) for row in want for x in (row if isinstance(row, (list, tuple)) else [row])]
            assert [int(x) for x in g.ravel()] == flat, f"{name} at {sh.V} voices: state {what}"
    sh.finish(name)


def case_sineosc(ctx, oracle, sh, image):
    from zang_amd import modules as mod, zang
    L = oracle.lib()
    m = mod.SineOsc(sh.V, ctx)
    t = sh.target(sh.fbuf, sh.fcol) if image else sh.target()
    fr = zang.buffer(t.src) if image else zang.constant(sh.gf)
    ph = 0.25 if image else 0.0
    sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], [], False, m.Params(SR, fr, zang.constant(ph)), zero_first=zf))
    ref = t.ref; rt = []
    for j, v in enumerate(sh.idx):
        st = oracle.SineOsc(); L.zo_sineosc_init(C.byref(st))
        for _, zf in sh.steps():
            sh.oracle_zero(L, oracle, t, j, zf)
            L.zo_sineosc_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), SR, oracle.buffer(t.col(j)) if image else oracle.constant(sh.freq[v]), oracle.constant(ph))
        rt.append(st.t)
    _check(sh, ctx, "SineOsc " + ("freq image" if image else "const"), t.o, ref, lambda: [("t", m.state()["t"][sh.idx], rt)])


def case_osc(ctx, oracle, sh, which, image):
    from zang_amd import modules as mod, zang
    L = oracle.lib()
    cls, ocls, init, paint = ((mod.PulseOsc, oracle.PulseOsc, L.zo_pulseosc_init, L.zo_pulseosc_paint) if which == "pulse" else
                              (mod.TriSawOsc, oracle.TriSawOsc, L.zo_trisawosc_init, L.zo_trisawosc_paint))
    m = cls(sh.V, ctx)
    t = sh.target(sh.fbuf, sh.fcol) if image else sh.target()
    fr = zang.buffer(t.src) if image else zang.constant(sh.gf)
    sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], [], False, m.Params(SR, fr, sh.gc), zero_first=zf))
    ref = t.ref; rs = []
    for j, v in enumerate(sh.idx):
        st = ocls(); init(C.byref(st))
        for _, zf in sh.steps():
            sh.oracle_zero(L, oracle, t, j, zf)
            paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), SR, oracle.buffer(t.col(j)) if image else oracle.constant(sh.freq[v]), float(sh.color[v]))
        rs.append((st.cnt, st.t if which == "trisaw" else 0.0))
    def states():
        gs = m.state()
        out = [("cnt", gs["cnt"][sh.idx], [r[0] for r in rs])]
        if which == "trisaw":
            out.append(("t", gs["t"][sh.idx], [r[1] for r in rs]))
        return out
    _check(sh, ctx, f"{which} osc " + ("freq image" if image else "const"), t.o, ref, states)


def case_sampler(ctx, oracle, sh):
    from zang_amd import modules as mod
    L = oracle.lib()
    sh.one_span()
    m = mod.Sampler(sh.V, ctx); o = sh.out()
    smp = m.Sample(1, 44100, m.signed16_lsb, sh.gpcm)
    rate = (sh.freq * np.float32(40.0)).astype(np.float32)
    gr = sh.pv(rate)
    for k in range(2):
        m.paint(sh.span(), [o], [], False, m.Params(gr, smp, 0, True), zero_first=(k == 0))
    ref = np.zeros((len(sh.idx), sh.F), np.float32); rt = []
    for j, v in enumerate(sh.idx):
        st = oracle.Sampler(); L.zo_sampler_init(C.byref(st))
        p = oracle.SamplerParams(float(rate[v]), 1, 44100, oracle.SAMPLE_S16, sh.pcm.ctypes.data_as(C.POINTER(C.c_uint8)), sh.pcm.size, 0, 1)
        for _ in range(2):
            L.zo_sampler_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), 0, C.byref(p))
        rt.append(st.t)
    _check(sh, ctx, "Sampler", o, ref, lambda: [("t", m.state()["t"][sh.idx], rt)])


def _env_params(oracle, on):
    return oracle.EnvelopeParams(SR, oracle.curve(3, 0.004), oracle.curve(3, 0.02), oracle.curve(3, 0.03), 0.6, int(on))


def case_envelope(ctx, oracle, sh):
    from zang_amd import modules as mod, zang
    L = oracle.lib()
    m = mod.Envelope(sh.V, ctx); o = sh.out()
    # one span: the second buffer keeps most voices on (decay -> sustain), every fifth releases.  Consecutive spans: a new note
    # at the first, on through the first four, every voice released from the fifth
    on1 = (np.arange(sh.V) % 5 != 0) if sh.geo.spans is None else np.zeros(sh.V, bool)
    off_at = 1 if sh.geo.spans is None else 4
    g_on1 = sh.pv(on1.astype(np.uint8))
    P = lambda on: m.Params(SR, zang.PaintCurve.cubed(0.004), zang.PaintCurve.cubed(0.02), zang.PaintCurve.cubed(0.03), 0.6, on)
    for k, zf in sh.steps((True, False)):
        m.paint(sh.span(), [o], [], k == 0, P(True if k < off_at else g_on1), zero_first=zf)
    ref = np.zeros((len(sh.idx), sh.F), np.float32); rs = []
    for j, v in enumerate(sh.idx):
        st = oracle.Envelope(); L.zo_envelope_init(C.byref(st))
        for k, _ in sh.steps((True, False)):
            L.zo_envelope_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), int(k == 0), C.byref(_env_params(oracle, True if k < off_at else on1[v])))
        rs.append((st.state, st.painter.t, st.painter.last_value, st.painter.start))
    def states():
        gs = m.state()
        return [(n, gs[n][sh.idx], [r[i] for r in rs]) for i, n in enumerate(("state", "t", "last_value", "start"))]
    _check(sh, ctx, "Envelope", o, ref, states)


def ref_decimator(oracle, s, e, zf_seq, ref, col, fake, in_place):
    """The oracle's carried Decimator paints of ONE voice onto ref (a [frames] row): -> its state.  in_place: the input IS ref,
    and ZERO_FIRST is what the reference's caller does -- zang.zero(span, out), then the paint with the same slice twice.  An
    entry of zf_seq is zero_first, or (s, e, zero_first) for a paint with a span of its own (Shared.pieces)."""
    L = oracle.lib()
    st = oracle.Decimator(); L.zo_decimator_init(C.byref(st))
    for zf in zf_seq:
        s, e, zf = zf if isinstance(zf, tuple) else (s, e, zf)
        if zf:
            L.zo_zero(s, e, oracle.fptr(ref))
        L.zo_decimator_paint(C.byref(st), s, e, oracle.fptr(ref), SR, oracle.fptr(ref if in_place else col), float(fake))
    return st


def case_decimator(ctx, oracle, sh):
    from zang_amd import modules as mod
    m = mod.Decimator(sh.V, ctx)
    t = sh.target(sh.ibuf, sh.icol)
    fake = (sh.freq * np.float32(8.0)).astype(np.float32)
    gfake = sh.pv(fake)
    sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], [], False, m.Params(SR, t.src, gfake), zero_first=zf))
    ref = t.ref; rs = []
    pieces = sh.pieces()
    for j, v in enumerate(sh.idx):
        st = ref_decimator(oracle, sh.s, sh.e, pieces, ref[j], sh.icol[j], fake[v], t.in_place)
        rs.append((st.dval, st.dcount))
    def states():
        gs = m.state()
        return [("dval", gs["dval"][sh.idx], [r[0] for r in rs]), ("dcount", gs["dcount"][sh.idx], [r[1] for r in rs])]
    _check(sh, ctx, "Decimator", t.o, ref, states)


def ref_filter(oracle, s, e, zf_seq, ref, col, ftype, cutoff, res, in_place, cutoff_in_place=False):
    """The oracle's carried Filter paints of ONE voice onto ref: -> its state.  `cutoff`: a float, or a [frames] column (a
    control image); in_place: the input IS ref; cutoff_in_place: the cutoff column IS ref."""
    L = oracle.lib()
    st = oracle.Filter(); L.zo_filter_init(C.byref(st))
    for zf in zf_seq:
        s, e, zf = zf if isinstance(zf, tuple) else (s, e, zf)          # (an entry with a span of its own: Shared.pieces)
        if zf:
            L.zo_zero(s, e, oracle.fptr(ref))
        cut = oracle.buffer(ref) if cutoff_in_place else (oracle.buffer(cutoff) if isinstance(cutoff, np.ndarray) else oracle.constant(cutoff))
        L.zo_filter_paint(C.byref(st), s, e, oracle.fptr(ref), oracle.fptr(ref if in_place else col), ftype, cut, oracle.constant(res))
    return st


def case_filter(ctx, oracle, sh, ftype, cutoff_image):
    from zang_amd import modules as mod, zang
    m = mod.Filter(sh.V, ctx)
    ctl = cutoff_image and sh.alias_ctl and sh.geo.in_place      # the cutoff image is the output; the input a separate image
    t = sh.target(sh.cbuf, sh.ccol) if ctl else sh.target(sh.ibuf, sh.icol)
    src = sh.ibuf if ctl else t.src
    cut = zang.buffer(t.src if ctl else sh.cbuf) if cutoff_image else zang.constant(sh.gc)
    sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], [], False, m.Params(src, ftype, cut, zang.constant(0.4)), zero_first=zf))
    ref = t.ref; rs = []
    pieces = sh.pieces()
    for j, v in enumerate(sh.idx):
        st = ref_filter(oracle, sh.s, sh.e, pieces, ref[j], sh.icol[j], ftype, sh.ccol[j] if cutoff_image else float(sh.color[v]), 0.4,
                        t.in_place and not ctl, bool(ctl))
        rs.append((st.l, st.b))
    def states():
        gs = m.state()
        return [("l", gs["l"][sh.idx], [r[0] for r in rs]), ("b", gs["b"][sh.idx], [r[1] for r in rs])]
    _check(sh, ctx, f"Filter type {ftype} " + ("cutoff image" if cutoff_image else "const") + (", the cutoff image painted onto" if ctl else ""), t.o, ref, states)


def case_echoes(ctx, oracle, sh, filtered):
    from zang_amd import modules as mod
    L = oracle.lib()
    F, D = sh.F, sh.D
    t = sh.target(sh.ibuf, sh.icol)
    n = len(sh.idx)
    ref = t.ref; rings = np.zeros((n, D), np.float32); rs = []
    t0 = np.zeros(F, np.float32); t1 = np.zeros(F, np.float32)
    if filtered:
        m = mod.FilteredEchoes(sh.V, D, ctx)
        sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], None, False, m.Params(t.src, 0.5, 0.2), zero_first=zf))
    else:
        m = mod.SimpleDelay(sh.V, D, ctx)
        sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], [], False, m.Params(t.src), zero_first=zf))
    for j in range(n):
        d = oracle.Delay(); L.zo_delay_init(C.byref(d), oracle.fptr(rings[j]), D)
        fl = oracle.Filter(); L.zo_filter_init(C.byref(fl))
        for _, zf in sh.steps():
            sh.oracle_zero(L, oracle, t, j, zf)
            if filtered:
                L.zo_filtered_echoes_paint(C.byref(d), C.byref(fl), sh.s, sh.e, oracle.fptr(ref[j]), oracle.fptr(t0), oracle.fptr(t1), oracle.fptr(t.col(j)), 0.5, 0.2)
            else:
                L.zo_simple_delay_paint(C.byref(d), sh.s, sh.e, oracle.fptr(ref[j]), oracle.fptr(t.col(j)))
        rs.append((d.index, fl.l, fl.b))
    def states():
        st = m.state()
        out = [("ring", st[0][sh.idx], rings), ("index", np.asarray(st[1])[sh.idx], [r[0] for r in rs])]
        if filtered:
            out += [("l", st[2]["l"][sh.idx], [r[1] for r in rs]), ("b", st[2]["b"][sh.idx], [r[2] for r in rs])]
        return out
    _check(sh, ctx, "FilteredEchoes" if filtered else "SimpleDelay", t.o, ref, states)


def case_nice(ctx, oracle, sh):
    from zang_amd import modules as mod
    L = oracle.lib()
    F = sh.F
    m = mod.NiceInstrument(sh.V, sh.gc, ctx); o = sh.out()
    off_at = 1 if sh.geo.spans is None else 4          # (consecutive spans: the note on through the first four, off from the fifth)
    for k, zf in sh.steps((True, False)):
        m.paint(sh.span(), [o], None, k == 0, m.Params(SR, sh.gf, k < off_at), zero_first=zf)
    ref = np.zeros((len(sh.idx), F), np.float32); rs = []
    t0 = np.zeros(F, np.float32); t1 = np.zeros(F, np.float32)
    for j, v in enumerate(sh.idx):
        st = oracle.NiceInstrument(); L.zo_nice_init(C.byref(st), float(sh.color[v]))
        for k, _ in sh.steps((True, False)):
            L.zo_nice_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), oracle.fptr(t0), oracle.fptr(t1), int(k == 0), SR, float(sh.freq[v]), int(k < off_at))
        rs.append((st.osc.cnt, st.flt.l, st.flt.b, st.env.state, st.env.painter.t, st.env.painter.last_value, st.env.painter.start))
    def states():
        gs = m.state()
        return [("osc.cnt", gs["osc"]["cnt"][sh.idx], [r[0] for r in rs]), ("flt.l", gs["flt"]["l"][sh.idx], [r[1] for r in rs]),
                ("flt.b", gs["flt"]["b"][sh.idx], [r[2] for r in rs]), ("env.state", gs["env"]["state"][sh.idx], [r[3] for r in rs]),
                ("env.t", gs["env"]["t"][sh.idx], [r[4] for r in rs]), ("env.last_value", gs["env"]["last_value"][sh.idx], [r[5] for r in rs]),
                ("env.start", gs["env"]["start"][sh.idx], [r[6] for r in rs])]
    _check(sh, ctx, "NiceInstrument", o, ref, states)


def case_pmosc(ctx, oracle, sh):
    from zang_amd import modules as mod
    L = oracle.lib()
    F = sh.F
    sh.one_span()
    rel = (0.1 + 0.4 * sh.u2).astype(np.float32)
    m = mod.PMOscInstrument(sh.V, sh.pv(rel), ctx); o = sh.out()
    m.paint(sh.span(), [o], None, True, m.Params(SR, sh.gf, True), zero_first=True)
    m.paint(sh.span(), [o], None, False, m.Params(SR, sh.gf, False))
    ref = np.zeros((len(sh.idx), F), np.float32); rs = []
    t = [np.zeros(F, np.float32) for _ in range(3)]
    for j, v in enumerate(sh.idx):
        st = oracle.PMOscInstrument(); L.zo_pmosc_init(C.byref(st), float(rel[v]))
        for k in range(2):
            L.zo_pmosc_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), oracle.fptr(t[0]), oracle.fptr(t[1]), oracle.fptr(t[2]), int(k == 0), SR, float(sh.freq[v]), int(k == 0))
        rs.append((st.carrier.t, st.modulator.t, st.env.state, st.env.painter.t, st.env.painter.last_value, st.env.painter.start))
    def states():
        gs = m.state()
        return [("carrier.t", gs["carrier"]["t"][sh.idx], [r[0] for r in rs]), ("modulator.t", gs["modulator"]["t"][sh.idx], [r[1] for r in rs]),
                ("env.state", gs["env"]["state"][sh.idx], [r[2] for r in rs]), ("env.t", gs["env"]["t"][sh.idx], [r[3] for r in rs]),
                ("env.last_value", gs["env"]["last_value"][sh.idx], [r[4] for r in rs]), ("env.start", gs["env"]["start"][sh.idx], [r[5] for r in rs])]
    _check(sh, ctx, "PMOscInstrument", o, ref, states)


def case_noise(ctx, oracle, sh, color, first_zf=True):
    """White / pink: ZERO_FIRST then ADD (the ADD form of the white frame ranges goes through a module-owned image).  Three
    sampled voices start from crafted generator states: a multi-draw sample inside the first paint, near its end, and inside
    the second paint."""
    from zang_amd import modules as mod
    L = oracle.lib()
    first = 5000
    d0, d1, d2 = noise_draws(sh, "noise")                                               # (1,024 frames: draws 77, 1001, 1024 + 515)
    m = mod.Noise(sh.V, ctx, first_seed=first); o = sh.out(fill=0.0)                    # (the first paint may be an ADD)
    crafted = {int(sh.idx[3]): _crafted_noise_state(d0, 1), int(sh.idx[-3]): _crafted_noise_state(d1, 2), int(sh.idx[len(sh.idx) // 2]): _crafted_noise_state(d2, 3)}
    st = m.state()
    for v, r in crafted.items():
        st["r"][v] = r
    taps = np.random.default_rng(9).uniform(-0.5, 0.5, (sh.V, 7)).astype(np.float32)
    taps[::3] = 0.0
    st["b"][:] = taps
    m.set_state(st)
    for _, zf in sh.steps((first_zf, False)):
        m.paint(sh.span(), [o], [], False, m.Params(color), zero_first=zf)
    ref = np.zeros((len(sh.idx), sh.F), np.float32); rs = []
    for j, v in enumerate(sh.idx):
        nz = oracle.Noise(); L.zo_noise_init(C.byref(nz), first + int(v))
        if int(v) in crafted:
            for i in range(4):
                nz.r[i] = crafted[int(v)][i]
        for i in range(7):
            nz.b[i] = float(taps[v, i])
        for _ in sh.steps((first_zf, False)):
            L.zo_noise_paint(C.byref(nz), sh.s, sh.e, oracle.fptr(ref[j]), color)
        rs.append(list(nz.r))
    def states():
        gs = m.state()
        return [("r", gs["r"][sh.idx], rs), ("b (never written back, Noise.zig:68)", gs["b"][sh.idx], taps[sh.idx])]
    _check(sh, ctx, "Noise " + ("pink" if color else "white"), o, ref, states)


def case_noise_filter(ctx, oracle, sh, color):
    from zang_amd import modules as mod
    L = oracle.lib()
    first = 9000
    d0, d1 = noise_draws(sh, "filter")                                                  # (1,024 frames: draws 300, 1024 + 9)
    cutoff = (0.02 + 0.5 * sh.u2).astype(np.float32); res = (0.9 * sh.u3).astype(np.float32)
    m = mod.NoiseFilter(sh.V, ctx, first_seed=first); o = sh.out()
    crafted = {int(sh.idx[5]): _crafted_noise_state(d0, 4), int(sh.idx[-2]): _crafted_noise_state(d1, 5)}
    st = m.state()
    for v, r in crafted.items():
        st["noise"]["r"][v] = r
    m.set_state(st)
    gcut, gres = sh.pv(cutoff), sh.pv(res)
    for _, zf in sh.steps((True, False)):
        m.paint(sh.span(), [o], None, False, m.Params(color, mod.Filter.low_pass, gcut, gres), zero_first=zf)
    ref = np.zeros((len(sh.idx), sh.F), np.float32); rs = []
    temp = np.zeros(sh.F, np.float32)
    for j, v in enumerate(sh.idx):
        nz = oracle.Noise(); L.zo_noise_init(C.byref(nz), first + int(v))
        if int(v) in crafted:
            for i in range(4):
                nz.r[i] = crafted[int(v)][i]
        fl = oracle.Filter(); L.zo_filter_init(C.byref(fl))
        for _ in sh.steps((True, False)):
            L.zo_zero(sh.s, sh.e, oracle.fptr(temp))
            L.zo_noise_paint(C.byref(nz), sh.s, sh.e, oracle.fptr(temp), color)
            L.zo_filter_paint(C.byref(fl), sh.s, sh.e, oracle.fptr(ref[j]), oracle.fptr(temp), oracle.FILTER_LOW_PASS, oracle.constant(cutoff[v]), oracle.constant(res[v]))
        rs.append((list(nz.r), fl.l, fl.b))
    def states():
        gs = m.state()
        return [("noise.r", gs["noise"]["r"][sh.idx], [r[0] for r in rs]), ("flt.l", gs["flt"]["l"][sh.idx], [r[1] for r in rs]),
                ("flt.b", gs["flt"]["b"][sh.idx], [r[2] for r in rs])]
    _check(sh, ctx, "Noise->Filter fused, " + ("pink" if color else "white"), o, ref, states)


def case_curve(ctx, oracle, sh, function):
    from zang_amd import modules as mod
    L = oracle.lib()
    sh.one_span()
    rng = np.random.default_rng(97)
    ts = np.cumsum(rng.uniform(0.0004, 0.006, 24)).astype(np.float32); ts[0] = 0.0
    vals = rng.uniform(-1, 1, 24).astype(np.float32)
    ts[5] = ts[4]
    nodes = np.stack([vals, ts], axis=1).astype(np.float32)
    carr = (oracle.CurveNode * len(nodes))(*[oracle.CurveNode(float(v), float(t)) for v, t in nodes])
    nic1 = (np.arange(sh.V) % 7 == 0)
    m = mod.Curve(sh.V, ctx); o = sh.out()
    gn = _dev(nodes)
    m.paint(sh.span(), [o], [], True, m.Params(SR, function, gn), zero_first=True)
    m.paint(sh.span(), [o], [], sh.pv(nic1.astype(np.uint8)), m.Params(SR, function, gn))
    ref = np.zeros((len(sh.idx), sh.F), np.float32); rs = []
    for j, v in enumerate(sh.idx):
        st = oracle.CurveModule(); L.zo_curve_init(C.byref(st))
        L.zo_curve_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), 1, SR, function, carr, len(nodes))
        L.zo_curve_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), int(nic1[v]), SR, function, carr, len(nodes))
        rs.append((st.t, st.current_song_note, st.current_song_note_offset, st.next_song_note))
    def states():
        gs = m.state()
        return [(n, gs[n][sh.idx], [r[i] for r in rs]) for i, n in enumerate(("t", "current_song_note", "current_song_note_offset", "next_song_note"))]
    _check(sh, ctx, f"Curve fn {function}", o, ref, states)


def case_cycle(ctx, oracle, sh, image):
    from zang_amd import modules as mod, zang
    L = oracle.lib()
    m = mod.Cycle(sh.V, ctx)
    t = sh.target(sh.fbuf, sh.fcol) if image else sh.target()
    sp = zang.buffer(t.src) if image else zang.constant(sh.gf)
    sh.paints(lambda k, zf: m.paint(sh.span(), [t.o], [], False, m.Params(SR, sp), zero_first=zf))
    ref = t.ref; rt = []
    for j, v in enumerate(sh.idx):
        st = oracle.Cycle(); L.zo_cycle_init(C.byref(st))
        for _, zf in sh.steps():
            sh.oracle_zero(L, oracle, t, j, zf)
            L.zo_cycle_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), SR, oracle.buffer(t.col(j)) if image else oracle.constant(sh.freq[v]))
        rt.append(st.t)
    _check(sh, ctx, "Cycle " + ("speed image" if image else "const"), t.o, ref, lambda: [("t", m.state()["t"][sh.idx], rt)])


def case_portamento(ctx, oracle, sh):
    from zang_amd import modules as mod, zang
    L = oracle.lib()
    sh.one_span()
    dur = (0.002 + 0.03 * sh.u2).astype(np.float32)
    goal0 = sh.freq; goal1 = (sh.freq * np.float32(1.5)).astype(np.float32)
    m = mod.Portamento(sh.V, ctx); o = sh.out()
    gcurve = zang.PaintCurve.cubed(sh.pv(dur))
    m.paint(sh.span(), [o], [], True, m.Params(SR, gcurve, sh.pv(goal0), True, False), zero_first=True)
    m.paint(sh.span(), [o], [], True, m.Params(SR, gcurve, sh.pv(goal1), True, True))
    ref = np.zeros((len(sh.idx), sh.F), np.float32); rs = []
    for j, v in enumerate(sh.idx):
        st = oracle.Portamento(); L.zo_portamento_init(C.byref(st))
        L.zo_portamento_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), 1, SR, oracle.curve(3, dur[v]), float(goal0[v]), 1, 0)
        L.zo_portamento_paint(C.byref(st), sh.s, sh.e, oracle.fptr(ref[j]), 1, SR, oracle.curve(3, dur[v]), float(goal1[v]), 1, 1)
        rs.append((st.painter.t, st.painter.last_value, st.painter.start))
    def states():
        gs = m.state()
        return [(n, gs[n][sh.idx], [r[i] for r in rs]) for i, n in enumerate(("t", "last_value", "start"))]
    _check(sh, ctx, "Portamento", o, ref, states)


def case_stateless(ctx, oracle, sh):
    """Gate (bit-exact index arithmetic) and Distortion (both types), frame-chunked kernels without state."""
    from zang_amd import modules as mod
    L = oracle.lib()
    sh.one_span()
    on = (np.arange(sh.V) % 3 != 1)
    g = mod.Gate(sh.V, ctx); o = sh.out()
    gon = sh.pv(on.astype(np.uint8))
    for k in range(2):
        g.paint(sh.span(), [o], [], False, g.Params(gon), zero_first=(k == 0))
    ref = np.zeros((len(sh.idx), sh.F), np.float32)
    for j, v in enumerate(sh.idx):
        for _ in range(2):
            L.zo_gate_paint(sh.s, sh.e, oracle.fptr(ref[j]), int(on[v]))
    _check(sh, ctx, "Gate", o, ref, lambda: [])
    for dtype in (0, 1):
        d = mod.Distortion(sh.V, ctx)
        t = sh.target(sh.ibuf, sh.icol)
        ing = (0.1 + 0.85 * sh.u2).astype(np.float32); outg = (0.2 + 0.7 * sh.u3).astype(np.float32)
        ging, goutg = sh.pv(ing), sh.pv(outg)
        sh.paints(lambda k, zf: d.paint(sh.span(), [t.o], [], False, d.Params(t.src, dtype, ging, goutg, 0.1), zero_first=zf))
        ref = t.ref
        for j, v in enumerate(sh.idx):
            for _, zf in sh.steps():
                sh.oracle_zero(L, oracle, t, j, zf)
                L.zo_distortion_paint(sh.s, sh.e, oracle.fptr(ref[j]), oracle.fptr(t.col(j)), dtype, float(ing[v]), float(outg[v]), 0.1)
        _check(sh, ctx, f"Distortion type {dtype}", t.o, ref, lambda: [])


CASES = {
    "sineosc_const": lambda c, o, s: case_sineosc(c, o, s, False),
    "sineosc_image": lambda c, o, s: case_sineosc(c, o, s, True),
    "pulse_const": lambda c, o, s: case_osc(c, o, s, "pulse", False),
    "pulse_image": lambda c, o, s: case_osc(c, o, s, "pulse", True),
    "trisaw_const": lambda c, o, s: case_osc(c, o, s, "trisaw", False),
    "trisaw_image": lambda c, o, s: case_osc(c, o, s, "trisaw", True),
    "sampler": case_sampler,
    "envelope": case_envelope,
    "decimator": case_decimator,
    "filter_lowpass_const": lambda c, o, s: case_filter(c, o, s, 1, False),
    "filter_bandpass_const": lambda c, o, s: case_filter(c, o, s, 2, False),
    "filter_notch_image": lambda c, o, s: case_filter(c, o, s, 4, True),
    "filtered_echoes": lambda c, o, s: case_echoes(c, o, s, True),
    "simple_delay": lambda c, o, s: case_echoes(c, o, s, False),
    "nice": case_nice,
    "pmosc": case_pmosc,
    "noise_white": lambda c, o, s: case_noise(c, o, s, 0),
    "noise_white_add": lambda c, o, s: case_noise(c, o, s, 0, first_zf=False),
    "noise_pink": lambda c, o, s: case_noise(c, o, s, 1),
    "noise_filter_white": lambda c, o, s: case_noise_filter(c, o, s, 0),
    "noise_filter_pink": lambda c, o, s: case_noise_filter(c, o, s, 1),
    "curve_linear": lambda c, o, s: case_curve(c, o, s, 0),
    "curve_smoothstep": lambda c, o, s: case_curve(c, o, s, 1),
    "cycle_const": lambda c, o, s: case_cycle(c, o, s, False),
    "cycle_image": lambda c, o, s: case_cycle(c, o, s, True),
    "portamento": case_portamento,
    "stateless": case_stateless,
}

# the cases that read an image: what the in_place geometry runs (an input image IS the output; the image-controlled oscillators and
# Cycle paint onto their control image; Filter with a cutoff image once onto its input and once onto its cutoff image)
IMAGE_CASES = ["sineosc_image", "pulse_image", "trisaw_image", "decimator", "filter_lowpass_const", "filter_bandpass_const",
               "filter_notch_image", "filtered_echoes", "simple_delay", "cycle_image", "stateless"]
