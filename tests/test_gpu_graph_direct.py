"""GPU: the direct replay of a ZH_CAPTURE_COALESCE capture (csrc/ctx.hip zh_graph_launch, form row `graph_direct`).  A capture that
recorded nothing but held-back constant-frequency oscillator batches is replayed by enqueuing one launch per batch -- the live counters
read, the other buffer written, one flip -- instead of the recorded hipGraph, which splits the last batch so that it ends on the counter
buffer it began on.  Every replay is compared bit for bit, images and carried state, with a twin capture replayed through the recorded
graph (graph_direct=0), and the driver's shape with the oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu
SR = 48000.0


class Twins:
    """Two copies of the same modules and images on one context (side stream): `d` is replayed directly, `r` through the recorded graph."""

    def __init__(self, kind, V, frames, n_mods, n_imgs):
        import torch
        import zang_amd
        from zang_amd import modules as mod, zang, workloads
        self.zang, self.V, self.frames = zang, V, frames
        freq, color, u2, _ = workloads.voice_params(2, 0, V)
        self.stream = torch.cuda.Stream()
        with torch.cuda.stream(self.stream):
            self.c = zang_amd.Context(0)
            Osc = mod.PulseOsc if kind == "pulse" else mod.TriSawOsc
            fr = [torch.from_numpy((freq * (1.0 + 0.5 * k * u2)).astype(np.float32)).cuda() for k in range(n_mods)]
            col = torch.from_numpy(color).cuda()
            self.sets = []
            for _ in range(2):
                ms = [Osc(V, self.c) for _ in range(n_mods)]
                self.sets.append({"m": ms, "P": [m.Params(SR, zang.constant(f), col) for m, f in zip(ms, fr)],
                                  "img": [self.c.image(frames, V, fill=0.25) for _ in range(n_imgs)]})
            for s in self.sets:                               # an unflagged paint first: the constants table is stored
                for m, P in zip(s["m"], s["P"]):
                    m.paint(zang.Span(0, frames), [s["img"][0]], [], False, P, zero_first=True)
            self.c.sync()

    def paint(self, s, k, i, span=None, zero_first=True, flagged=True):
        span = span or self.zang.Span(0, self.frames)
        s["m"][k].paint(span, [s["img"][i]], [], False, s["P"][k], zero_first=zero_first, params_unchanged=flagged)

    def capture(self, seq):
        import torch
        with torch.cuda.stream(self.stream):
            return [self.c.capture(lambda s=s: seq(s), coalesce=True) for s in self.sets]

    def launch(self, monkeypatch, gd, gr):
        import torch
        with torch.cuda.stream(self.stream):
            util.set_form(monkeypatch, graph_direct=1)
            gd.launch()
            util.set_form(monkeypatch, graph_direct=0)
            gr.launch()
            util.del_form(monkeypatch, "graph_direct")

    def eager(self, fn):
        import torch
        with torch.cuda.stream(self.stream):
            for s in self.sets:
                fn(s)

    def check(self, what):
        import torch
        self.c.sync()
        d, r = self.sets
        for q, (x, y) in enumerate(zip(d["img"], r["img"])):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, "image", q)
        for k, (a, b) in enumerate(zip(d["m"], r["m"])):
            assert np.asarray(a.state()).tobytes() == np.asarray(b.state()).tobytes(), (what, "module", k)

    def close(self, *graphs):
        for g in graphs:
            g.close()
        self.c.close()


def _kernels(monkeypatch, g, direct):
    util.set_form(monkeypatch, graph_direct=direct)
    ks = g.kernels()
    util.del_form(monkeypatch, "graph_direct")
    return ks


@pytest.mark.parametrize("kind", ["pulse", "trisaw"])
@pytest.mark.parametrize("K", [1, 19, 20, 33, 1000])
def test_direct_replay_equals_the_recorded_graph(kind, K, monkeypatch):
    """K paints of one module into K distinct images: one launch per 32 buffers replayed directly (20 -> one launch of 20, 1,000 -> 32),
    the recorded graph unchanged (20 -> two of 10); three replays with eager paints between them, same bits and counters as the graph"""
    V, frames = (2048, 1024) if K <= 33 else (256, 256)
    t = Twins(kind, V, frames, 1, K)
    gd, gr = t.capture(lambda s: [t.paint(s, 0, i) for i in range(K)])
    assert gd.info() == gr.info()
    want = {1: [("k_osc_const4", 1)], 19: [("k_osc_const4[batch]", 1)], 20: [("k_osc_const4[batch]", 1)],
            33: [("k_osc_const4[batch]", 1), ("k_osc_const4", 1)], 1000: [("k_osc_const4[batch]", 32)]}[K]
    assert _kernels(monkeypatch, gd, 1) == want, (K, gd.kernels())
    assert _kernels(monkeypatch, gd, 0) == _kernels(monkeypatch, gr, 0)
    assert sum(n for _, n in _kernels(monkeypatch, gr, 0)) == gr.info()[2]
    for rep in range(3):
        t.launch(monkeypatch, gd, gr)
        t.check((K, rep))
        if rep == 0:                                          # an eager paint between replays: one flip
            t.eager(lambda s: t.paint(s, 0, 0, t.zang.Span(0, 77)))
        if rep == 1:                                          # a flagged eager paint: the table form, one flip
            t.eager(lambda s: t.paint(s, 0, K - 1, t.zang.Span(3, 200), zero_first=False))
        t.check((K, rep, "eager"))
    t.close(gd, gr)


@pytest.mark.parametrize("kind", ["pulse", "trisaw"])
def test_two_graphs_of_one_module_alternate(kind, monkeypatch):
    """two captures of one module (20 and 7 paints, an odd count) replayed in turn, with eager paints between: each replay starts from
    whatever the other one or the eager paint left"""
    t = Twins(kind, 1024, 1024, 1, 27)
    g1 = t.capture(lambda s: [t.paint(s, 0, i) for i in range(20)])
    g2 = t.capture(lambda s: [t.paint(s, 0, i) for i in range(20, 27)])
    for rep, g in enumerate((g1, g2, g1, g1, g2, g2, g1)):
        t.launch(monkeypatch, *g)
        t.check(rep)
        if rep % 3 == 1:
            t.eager(lambda s: t.paint(s, 0, 3, t.zang.Span(0, 500)))
            t.check((rep, "eager"))
    t.close(*g1, *g2)


@pytest.mark.parametrize("kind", ["pulse", "trisaw"])
def test_two_modules_interleaved_in_one_capture(kind, monkeypatch):
    """two modules painted in turn (each paint ends the other's batch: one-buffer items), then in runs (batches of 3 and 4 buffers),
    and a span of another length (a new batch)"""
    t = Twins(kind, 1024, 1024, 2, 16)

    def seq(s):
        for i in range(6):
            t.paint(s, i % 2, i)
        for i in range(6, 9):
            t.paint(s, 0, i)
        for i in range(9, 13):
            t.paint(s, 1, i)
        for i in range(13, 16):
            t.paint(s, 0, i, t.zang.Span(0, 640))
    gd, gr = t.capture(seq)
    assert _kernels(monkeypatch, gd, 1) == [("k_osc_const4", 6), ("k_osc_const4[batch]", 3)], gd.kernels()
    for rep in range(3):
        t.launch(monkeypatch, gd, gr)
        t.check(rep)
        t.eager(lambda s: t.paint(s, 1, 2, t.zang.Span(0, 33)))
    t.close(gd, gr)


@pytest.mark.parametrize("other", ["zero", "copy", "filter", "setup_form"])
def test_a_capture_with_other_work_replays_the_recorded_graph(other, monkeypatch):
    """a capture that also recorded a basics call, a zh_copy, a non-oscillator paint or an oscillator paint that is not held back has no
    direct plan: zh_graph_kernels names the recorded launches whatever graph_direct says, and the replay is the graph's"""
    import torch
    from zang_amd import modules as mod
    t = Twins("pulse", 1024, 1024, 1, 22)
    with torch.cuda.stream(t.stream):
        flts = [mod.Filter(t.V, t.c) for _ in t.sets]
    for s, f in zip(t.sets, flts):
        s["flt"] = f
    sp = t.zang.Span(0, t.frames)

    def seq(s):
        for i in range(10):
            t.paint(s, 0, i)
        if other == "zero":
            t.zang.zero(t.zang.Span(0, 64), s["img"][20], t.c)
        elif other == "copy":
            t.zang.copy(sp, s["img"][20], s["img"][21], t.c)
        elif other == "filter":
            s["flt"].paint(sp, [s["img"][20]], [], False, s["flt"].Params(s["img"][21], s["flt"].low_pass, t.zang.constant(0.3), t.zang.constant(0.5)),
                           zero_first=True)
        else:
            t.paint(s, 0, 20, flagged=False)
        for i in range(10, 20):
            t.paint(s, 0, i)
    gd, gr = t.capture(seq)
    kd = _kernels(monkeypatch, gd, 1)
    assert kd == _kernels(monkeypatch, gd, 0) and sum(n for _, n in kd) > 2, kd
    if other != "setup_form":
        assert any(not k.startswith("k_osc_const4") for k, _ in kd), kd
    for rep in range(2):
        t.launch(monkeypatch, gd, gr)
        t.check(rep)
    t.close(gd, gr)


def test_a_module_destroyed_after_capture_refuses_the_direct_replay(monkeypatch):
    import torch
    from zang_amd import abi
    t = Twins("pulse", 512, 1024, 2, 8)
    gd, gr = t.capture(lambda s: [t.paint(s, i % 2, i) for i in range(8)])
    assert _kernels(monkeypatch, gd, 1) == [("k_osc_const4", 8)]
    with torch.cuda.stream(t.stream):
        for s in t.sets:
            s["m"][1].close()
        util.set_form(monkeypatch, graph_direct=1)
        assert t.c.lib.zh_graph_launch(t.c.handle, gd.handle) == abi.ZH_ERR_INVALID
        util.set_form(monkeypatch, graph_direct=0)
        assert t.c.lib.zh_graph_launch(t.c.handle, gr.handle) == abi.ZH_ERR_INVALID
    t.close(gd, gr)


@pytest.mark.parametrize("K", [19, 20])
def test_the_drivers_capture_replayed_directly_matches_oracle(K, oracle):
    """bench.py's pulseosc graph (K zero+paint steps of 4,096 voices over distinct images), replayed directly three times (the default
    form): every image equals the oracle's buffer of that step and the carried counters the oracle's -- on every 8th voice"""
    import torch
    import zang_amd
    from zang_amd import modules as mod, zang, workloads
    V, F = 4096, 1024
    freq, color, _, _ = workloads.voice_params(2, 0, V)
    L = oracle.lib()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        m = mod.PulseOsc(V, c2)
        fr, col = torch.from_numpy(freq).cuda(), torch.from_numpy(color).cuda()
        ring = [c2.image(F, V) for _ in range(K)]
        sp = zang.Span(0, F)
        P = m.Params(SR, zang.constant(fr), col)
        m.paint(sp, [ring[0]], [], False, P, zero_first=True)
        c2.sync()
        g = c2.capture(lambda: [m.paint(sp, [o], [], False, P, zero_first=True, params_unchanged=True) for o in ring], coalesce=True)
        assert g.kernels() == [("k_osc_const4[batch]", 1)] and g.info()[1:] == (K, 2), (g.kernels(), g.info())
        for _ in range(3):
            g.launch()
        c2.sync()
        got = [util.from_image(o)[::8] for o in ring]
        cnt = m.state()["cnt"][::8].copy()
        g.close(); c2.close()
    ref = np.zeros(F, np.float32)
    for q, v in enumerate(range(0, V, 8)):
        st = oracle.PulseOsc(); L.zo_pulseosc_init(C.byref(st))
        for step in range(1 + 3 * K):
            ref[:] = 0
            L.zo_pulseosc_paint(C.byref(st), 0, F, oracle.fptr(ref), SR, oracle.constant(freq[v]), float(color[v]))
            if step >= 1 + 2 * K:
                util.assert_bitexact(got[step - 1 - 2 * K][q], ref, f"K={K} voice {v} step {step}")
        assert int(cnt[q]) == int(st.cnt), (K, v)
