"""GPU: sample kits -- zh_sample_kit, zh_sampler_paint_kit_spans / zh_sampler_paint_kit (k_sampler_kit_spans: a Sampler lane whose
sample, channel, rate and loop flag are its own) and SamplePlayer -- against zo_sampler_paint called once per voice and sub-span
with that sub-span's sample descriptor on host copies of the same bytes (tests/sample_kit_cases.py), and against the per-format
kernels on one kit entry.  Everything on bits: the uint32 views of the images and of `t`."""
import ctypes as C

import numpy as np
import pytest

from tests import sample_kit_cases as sk
from tests import util

pytestmark = pytest.mark.gpu
FIELDS = ("sample_rate", "loop", "sample", "channel")


@pytest.fixture(scope="module")
def kit(ctx):
    from zang_amd.samplekit import SampleKit
    k = SampleKit(ctx, sk.kit_samples())
    yield k
    k.close()


def _values(tb, names=FIELDS):
    return {n: ((tb[n], None) if n == "sample_rate" else (None, tb[n])) for n in names}


def _table(m, tb, names=FIELDS):
    return m.kit_span_table(tb["count"], tb["start"], tb["end"], tb["nic"], _values(tb, names))


def _set_t(m, t):
    st = m.state(); st["t"] = t; m.set_state(st)


@pytest.mark.parametrize("V", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("zero_first", [False, True], ids=["add", "zero_first"])
def test_span_paint_equals_the_oracle_per_sub_span(ctx, oracle, kit, V, zero_first):
    """Two consecutive buffers with carried state: every wave holds all four formats, the empty sample, the out-of-range index
    and channels past the sample's in one sub-span; the second buffer's first sub-spans carry `t` into another sample."""
    from zang_amd import modules as mod, zang
    samples = sk.kit_samples()
    m = mod.Sampler(V, ctx)
    t_ref = sk.start_t(V, 5 + V)
    _set_t(m, t_ref)
    rng = np.random.default_rng(77 + V)
    for b in range(2):
        tb = sk.tables(V, 1000 * V + b, second=b == 1)
        base = rng.uniform(-1.0, 1.0, (V, sk.ROWS)).astype(np.float32)
        ref, t_ref = sk.reference(oracle, samples, tb, t_ref, base.copy(), zero_first)
        out = util.to_image(base)
        m.paint_kit_spans(zang.Span(*sk.SPAN), [out], None, m.KitParams(kit, 1.0, 99, 99, False), _table(m, tb), zero_first=zero_first)
        ctx.sync()
        assert ctx.last_form() == ["k_sampler_kit_spans"], ctx.last_form()
        util.assert_bitexact(util.from_image(out), ref, f"V={V} buffer {b}")
        util.assert_bitexact(m.state()["t"].astype(np.float32), t_ref, f"V={V} t after buffer {b}")
    m.close()


@pytest.mark.parametrize("mode", ["broadcast", "per_voice"])
def test_fields_without_a_span_array_take_the_params(ctx, oracle, kit, mode):
    """broadcast: no span arrays at all (span_params NULL), one sample / channel / rate / loop for every voice.  per_voice: rate and
    loop per sub-span, sample and channel from per-voice device arrays."""
    import torch
    from zang_amd import modules as mod, zang
    V = 65
    samples = sk.kit_samples()
    tb = sk.tables(V, 4242)
    m = mod.Sampler(V, ctx)
    t_ref = sk.start_t(V, 9)
    _set_t(m, t_ref)
    if mode == "broadcast":
        dflt = {"sample": 3, "channel": 2, "sample_rate": np.float32(30000.0), "loop": 1}
        params = m.KitParams(kit, 30000.0, 3, 2, True)
        names = ()
    else:
        dflt = {"sample": (np.arange(V) * 3 % 8).astype(np.uint32), "channel": (np.arange(V) % 3).astype(np.uint32)}
        params = m.KitParams(kit, 1.0, torch.from_numpy(dflt["sample"].astype(np.int32)).cuda(), torch.from_numpy(dflt["channel"].astype(np.int32)).cuda(), False)
        names = ("sample_rate", "loop")
    lean = {k: (v if k in ("count", "start", "end", "nic") or k in names else None) for k, v in tb.items()}
    base = util.rng_buffers(3, V, sk.ROWS)
    ref, t_ref = sk.reference(oracle, samples, lean, t_ref, base.copy(), False, dflt=dflt)
    out = util.to_image(base)
    table = m.kit_span_table(tb["count"], tb["start"], tb["end"], tb["nic"], _values(tb, names) if names else None)
    m.paint_kit_spans(zang.Span(*sk.SPAN), [out], None, params, table)
    ctx.sync()
    util.assert_bitexact(util.from_image(out), ref, mode)
    util.assert_bitexact(m.state()["t"].astype(np.float32), t_ref, mode + " t")
    assert not sk.same_bits(ref, base)
    m.close()


@pytest.mark.parametrize("V", [1, 64, 65])
def test_uniform_paint_equals_the_oracle(ctx, oracle, kit, V):
    """zh_sampler_paint_kit: V Sampler instances, each with its own sample, channel, rate, loop flag and note_id_changed, painting
    the span twice (ADD, then ZERO_FIRST) with carried state"""
    import torch
    from zang_amd import modules as mod, zang
    samples = sk.kit_samples()
    rng = np.random.default_rng(31 + V)
    m = mod.Sampler(V, ctx)
    t_ref = sk.start_t(V, 12 + V)
    _set_t(m, t_ref)
    S, E = sk.SPAN
    for b in range(2):
        one = sk.tables(V, 77 * V + b)
        tb = {"count": np.ones(V, np.uint32), "start": np.full((1, V), S, np.uint32), "end": np.full((1, V), E, np.uint32),
              "nic": one["nic"][:1], **{n: one[n][b:b + 1] for n in FIELDS}}
        base = rng.uniform(-1.0, 1.0, (V, sk.ROWS)).astype(np.float32)
        ref, t_ref = sk.reference(oracle, samples, tb, t_ref, base.copy(), b == 1)
        out = util.to_image(base)
        dev32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()
        params = m.KitParams(kit, util.dev(tb["sample_rate"][0]), dev32(tb["sample"][0]), dev32(tb["channel"][0]), util.dev(tb["loop"][0].astype(np.uint8)))
        m.paint_kit(zang.Span(S, E), [out], [], util.dev(tb["nic"][0]), params, zero_first=b == 1)
        ctx.sync()
        assert ctx.last_form() == ["k_sampler_kit"], ctx.last_form()
        util.assert_bitexact(util.from_image(out), ref, f"V={V} paint {b}")
        util.assert_bitexact(m.state()["t"].astype(np.float32), t_ref, f"V={V} t after paint {b}")
    m.close()


def test_one_entry_equals_the_per_format_kernels(ctx, kit):
    """Every voice on kit entry i, channel c: paint_kit_spans == zh_sampler_paint_spans given zh_sample_kit_sample(kit, i) and that
    channel on the same table (rate and loop per sub-span), image and state, for every entry and valid channel."""
    from zang_amd import abi, modules as mod, zang
    from zang_amd.runtime import as_buf, as_f32
    V = 65
    samples = sk.kit_samples()
    tb = sk.tables(V, 909)
    for i, (nch, _, _, _) in enumerate(samples):
        for c in range(nch):
            a, b = mod.Sampler(V, ctx), mod.Sampler(V, ctx)
            t0 = sk.start_t(V, 40 + i)
            _set_t(a, t0); _set_t(b, t0)
            base = util.rng_buffers(50 + i, V, sk.ROWS)
            out_a, out_b = util.to_image(base), util.to_image(base)
            a.paint_kit_spans(zang.Span(*sk.SPAN), [out_a], None, a.KitParams(kit, 1.0, i, c, False), _table(a, tb, ("sample_rate", "loop")))
            table = b.span_table(tb["count"], tb["start"], tb["end"], tb["nic"], _values(tb, ("sample_rate", "loop")))
            ctb, sp = table.device(ctx.device, ["sample_rate", "loop"])
            cp = abi.SamplerParams(as_f32(1.0), kit.sample(i), c, 0, 0)
            outs = (abi.Buf * 1)(as_buf(out_b))
            abi.check(ctx.lib.zh_sampler_paint_spans(b.handle, sk.SPAN[0], sk.SPAN[1], outs, None, C.byref(cp), sp, C.byref(ctb), abi.PAINT_ADD), "paint_spans")
            ctx.sync()
            util.assert_bitexact(util.from_image(out_a), util.from_image(out_b), f"entry {i} channel {c}")
            util.assert_bitexact(a.state()["t"].astype(np.float32), b.state()["t"].astype(np.float32), f"entry {i} channel {c} t")
            a.close(); b.close()
    s = kit.sample(6)
    assert (s.num_channels, s.sample_rate, s.format, s.data_len) == (2, 44100, 2, 29 * 6 + 5) and s.data
    n = C.c_uint32()
    assert ctx.lib.zh_sample_kit_count(kit.handle, C.byref(n)) == 0 and n.value == 7 == kit.count


def test_a_captured_kit_span_paint_replays_with_the_state_flip(oracle):
    """one kit span paint recorded in a graph and replayed twice == two direct paints (image and `t`)"""
    import torch
    import zang_amd
    from zang_amd import modules as mod, zang
    from zang_amd.samplekit import SampleKit
    V = 65
    tb = sk.tables(V, 5150)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)                      # binds to the side stream (capture needs a non-default stream)
        k2 = SampleKit(c2, sk.kit_samples())
        me, mg = mod.Sampler(V, c2), mod.Sampler(V, c2)
        base = util.rng_buffers(8, V, sk.ROWS)
        out_e, out_g = util.to_image(base), util.to_image(base)
        tab_e, tab_g = _table(me, tb), _table(mg, tb)
        tab_g.device(c2.device, list(FIELDS))         # uploaded before the capture records
        paint = lambda m, out, tab: m.paint_kit_spans(zang.Span(*sk.SPAN), [out], None, m.KitParams(k2, 1.0, 0, 0, False), tab)
        paint(me, out_e, tab_e); paint(me, out_e, tab_e)
        c2.sync()
        g = c2.capture(lambda: paint(mg, out_g, tab_g))
        g.launch(); g.launch()
        c2.sync()
        assert torch.equal(out_e.view(torch.int32), out_g.view(torch.int32))
        assert np.array_equal(me.state()["t"].view(np.uint32), mg.state()["t"].view(np.uint32))
        assert not torch.equal(out_e, util.to_image(base))
        g.close(); me.close(); mg.close(); k2.close()
        c2.close()


# ------------------------------------------------------------------ SamplePlayer
class _Note(C.Structure):                          # zang_amd.samplekit.NOTE_PARAMS
    _fields_ = [("sample_rate", C.c_float), ("sample", C.c_uint32), ("channel", C.c_uint32), ("loop", C.c_uint32), ("note_on", C.c_uint32)]


N, P, F, B = 3, 4, 96, 4


def _pushes():
    """per buffer (player, frame, note_id, sample, rate, channel, loop) in push order: 33 on player 1 in buffer 1 (the queue takes
    32), a reversed looping note, a note on the empty sample, notes that outlast their buffer"""
    rng = np.random.default_rng(20261018)
    out, nid = [], 1
    for b in range(B):
        ev = []
        for j in range(N):
            if j == 1 and b == 1:
                for k in range(33):
                    ev.append((j, 2 * k + 1, nid, k % 7, float(np.float32(rng.uniform(20000.0, 60000.0))), k % 2, k % 3 == 0)); nid += 1
                continue
            for f in sorted(rng.integers(0, F - 8, int(rng.integers(0, 4))).tolist()):
                ev.append((j, f, nid, int(rng.integers(0, 7)), float(np.float32(rng.choice([44100.0, 22050.0, 48000.0, 31000.0]))),
                           int(rng.integers(0, 2)), bool(rng.integers(0, 2)))); nid += 1
        if b == 0:
            ev.append((0, F - 7, nid, 1, -33075.0, 1, True)); nid += 1          # reversed, looping, carried into the next buffer
            ev.append((2, F - 3, nid, 4, 44100.0, 0, True)); nid += 1           # the empty sample
        out.append(ev)
    return out


@pytest.mark.parametrize("distort", [False, True], ids=["plain", "overdrive"])
def test_sample_player_equals_the_host_composition(ctx, oracle, kit, distort):
    """paint() == ImpulseQueue -> PolyphonyDispatcher -> Trigger per player on the host (zang_amd/notes.py), zo_sampler_paint per
    sub-span in voice order into one buffer, x 2.5, then the oracle's overdrive (example_sampler.zig:94-118)"""
    from zang_amd import notes
    from zang_amd.samplekit import SamplePlayer
    from zang_amd.zang import Span
    samples = sk.kit_samples()
    L = oracle.lib()
    player = SamplePlayer(ctx, N, kit, polyphony=P, sample_rate=44100, distort=distort)
    ns = notes.Notes(_Note)
    iq = [ns.ImpulseQueue() for _ in range(N)]
    pd = [ns.PolyphonyDispatcher(P)() for _ in range(N)]
    tr = [[notes.Trigger(_Note)() for _ in range(P)] for _ in range(N)]
    st = [[oracle.Sampler() for _ in range(P)] for _ in range(N)]
    loudest, most = 0.0, 0
    for b, ev in enumerate(_pushes()):
        for j, f, nid, smp, rate, ch, loop in ev:
            player.push(j, f, nid, smp, rate, ch, loop)
            iq[j].push(f, nid, _Note(rate, smp, ch, int(loop), 1))
        got = player.paint(F).cpu().numpy()
        want = np.zeros((N, F), np.float32)
        for j in range(N):
            poly = pd[j].dispatch(iq[j].consume())
            for i in range(P):
                ctr = tr[j][i].counter(Span(0, F), poly[i])
                n = 0
                while True:
                    r = tr[j][i].next(ctr)
                    if r is None:
                        break
                    n += 1
                    p = sk.oracle_params(oracle, samples, r.params.sample, r.params.channel, r.params.sample_rate, r.params.loop)
                    L.zo_sampler_paint(C.byref(st[j][i]), r.span.start, r.span.end, oracle.fptr(want[j]), int(r.note_id_changed), C.byref(p))
                most = max(most, n)
        want *= np.float32(2.5)
        if distort:
            mix, want = want, np.zeros((N, F), np.float32)
            for j in range(N):
                L.zo_distortion_paint(0, F, oracle.fptr(want[j]), oracle.fptr(mix[j]), 0, 0.9, 0.5, 0.0)
        util.assert_bitexact(got, want, f"buffer {b}")
        loudest = max(loudest, float(np.abs(want).max()))
    assert loudest > 0.05 and most >= 8
    assert player.overflows() == 0
    util.assert_bitexact(player.voices.state()["t"].astype(np.float32), np.array([x.t for row in st for x in row], np.float32), "t")
    player.close()


# ------------------------------------------------------------------ refusals
def test_refusals(ctx, kit):
    import torch
    import zang_amd
    from zang_amd import abi, modules as mod, zang
    from zang_amd.samplekit import SampleKit
    V = 8
    tb = sk.tables(V, 1)
    m = mod.Sampler(V, ctx)
    out = ctx.image(sk.ROWS, V)
    span = zang.Span(*sk.SPAN)
    good = m.KitParams(kit, 44100.0, 0, 0, False)
    assert m._paint_kit_spans(span, [out], None, good, _table(m, tb), abi.PAINT_ADD) == 0
    assert m._paint_kit_spans(span, [out], None, good, _table(m, tb), abi.PAINT_TOLERANT) == abi.ZH_ERR_UNSUPPORTED
    assert m._paint_kit_spans(span, [out[:50]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID      # too few rows
    assert m._paint_kit_spans(span, [out[:, :V - 1]], None, good, _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID  # too few voices
    with pytest.raises(abi.ZangHipError):
        m.paint_kit(span, [out[:50]], [], False, good)
    cp = abi.SamplerKitParams()                                          # a NULL kit
    ctb, sp = _table(m, tb).device(ctx.device, list(FIELDS))
    from zang_amd.runtime import as_buf
    outs = (abi.Buf * 1)(as_buf(out))
    assert ctx.lib.zh_sampler_paint_kit_spans(m.handle, span.start, span.end, outs, None, C.byref(cp), sp, C.byref(ctb), 0) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_sampler_paint_kit(m.handle, span.start, span.end, outs, None, abi.Bool(), C.byref(cp), 0) == abi.ZH_ERR_INVALID
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
        other = SampleKit(c2, sk.kit_samples())                          # a kit of another context
        assert m._paint_kit_spans(span, [out], None, m.KitParams(other, 44100.0, 0, 0, False), _table(m, tb), abi.PAINT_ADD) == abi.ZH_ERR_INVALID
        other.close(); c2.close()
    data = np.zeros(8, np.uint8)
    h = C.c_void_p()
    for nch, fmt, n in ((0, 1, 1), (1, 4, 1), (1, 1, 0)):               # no channels, a bad format, no samples
        s = abi.Sample(nch, 44100, fmt, 0, data.ctypes.data, data.size)
        assert ctx.lib.zh_sample_kit_create(ctx.handle, C.byref(s), n, C.byref(h)) == abi.ZH_ERR_INVALID
    s = abi.Sample(1, 44100, 1, 0, None, 4)                              # bytes promised, none given
    assert ctx.lib.zh_sample_kit_create(ctx.handle, C.byref(s), 1, C.byref(h)) == abi.ZH_ERR_INVALID
    ctx.sync()
    m.close()
