"""GPU: the FM voice over per-voice span tables (zh_fm_paint_spans, k_fm_spans in csrc/fm.hip) -- the synth's Trigger loop
(examples/example_fmsynth.zig:457-496) for every voice in one launch -- against the Trigger loop of tests/fm_reference.py over
three consecutive buffers with the state carried across; from tables a LiveVoiceBank makes out of pushed impulses; and recorded
once into a graph with its schedule.  130 voices in 26 instruments of 5, 1,024 frames; bit for bit throughout."""
import numpy as np
import pytest

from tests import fm_cases as fc
from tests import fm_reference as fr
from tests.util import assert_bitexact, from_image, to_image

pytestmark = pytest.mark.gpu
V, F, SR, GROUP, NI = fc.V, fc.F, fc.SR, fc.GROUP, fc.NI


def _instrument(ctx, patches=None):
    from zang_amd import modules as mod
    m = mod.FMInstrument(V, ctx, group=GROUP)
    m.set_patches(np.array(fc.patches() if patches is None else patches, np.uint32))
    return m


def _table(tb, device):
    from zang_amd.spans import SpanTable
    K = tb["start"].shape[0]
    return SpanTable.from_arrays(tb["count"], tb["start"][:K], tb["end"][:K], tb["freq"][:K], tb["note_on"][:K], tb["note_id_changed"][:K], device)


def _state(m):
    return np.frombuffer(m.state().tobytes(), fr.STATE_DTYPE).reshape(m.n_voices, 2)


def _assert_state(m, want, what):
    got = _state(m)
    for name in fr.STATE_DTYPE.names:
        assert_bitexact(got[name], want[name], f"{what}: state.{name}")


def test_three_buffers_against_the_helpers_trigger_loop(ctx):
    """tables with 0-3 sub-spans per voice: empty voices, sub-spans that touch, one that ends with the buffer, a single-frame one.
    Added onto a live image (frames outside the sub-spans stay), and with zero_first (they become 0)."""
    from zang_amd import zang
    x = fc.inputs()
    trem, vib = to_image(x["trem"]), to_image(x["vib"])
    a, z = _instrument(ctx), _instrument(ctx)
    span = zang.Span(0, F)
    for b, (tb, (m, c, painted, add_m, state)) in enumerate(zip(fc.span_tables(), fc.span_reference())):
        table = _table(tb, ctx.device)
        img_a, img_z = to_image(x["live"]), ctx.image(F, V, fill=9.0)
        a.paint_spans(span, [img_a], None, SR, trem, vib, table)
        z.paint_spans(span, [img_z], None, SR, trem, vib, table, zero_first=True)
        ctx.sync()
        assert_bitexact(from_image(img_a), fr.add_spans_into(x["live"], m, c, painted, add_m), f"buffer {b}, added")
        assert_bitexact(from_image(img_z), fr.add_spans_into(np.zeros((V, F), np.float32), m, c, painted, add_m), f"buffer {b}, zero_first")
        _assert_state(a, state, f"buffer {b}"); _assert_state(z, state, f"buffer {b}, zero_first")
    assert any("k_fm_spans" in name for name in ctx.last_form()), ctx.last_form()
    a.close(); z.close()


def test_a_sub_range_of_the_buffer(ctx):
    """span (0, 700) of the tables' first buffer cut to that range: frames from 700 on are not touched"""
    from zang_amd import zang
    x = fc.inputs()
    tb = {k: v.copy() for k, v in fc.span_tables()[0].items()}
    for v in range(V):                                                    # keep the sub-spans that lie inside [0, 700)
        keep = [k for k in range(tb["count"][v]) if tb["end"][k, v] <= 700]
        tb["count"][v] = len(keep)
        assert keep == list(range(len(keep)))
    ref = fr.FMRef(V, GROUP, fc.patches())
    m, c, painted, add_m = ref.paint_spans(0, 700, SR, x["trem"], x["vib"], tb)
    inst = _instrument(ctx)
    img = to_image(x["live"])
    inst.paint_spans(zang.Span(0, 700), [img], None, SR, to_image(x["trem"]), to_image(x["vib"]), _table(tb, ctx.device), zero_first=True)
    ctx.sync()
    want = x["live"].copy()
    want[:, :700] = fr.add_spans_into(np.zeros((V, F), np.float32), m, c, painted, add_m)[:, :700]
    assert_bitexact(from_image(img), want, "span (0, 700)")
    _assert_state(inst, ref.state(), "span (0, 700)")
    inst.close()


def test_split_operators_over_spans(ctx):
    from zang_amd import zang
    x = fc.inputs()
    tb = fc.span_tables()[0]
    m, c, painted, add_m, state = fc.span_reference()[0]
    base = np.random.default_rng(11).uniform(-1, 1, (2 * V, F)).astype(np.float32)
    inst_a, inst_z = _instrument(ctx), _instrument(ctx)
    img_a, img_z = to_image(base), ctx.image(F, 2 * V, fill=4.0)
    trem, vib, table = to_image(x["trem"]), to_image(x["vib"]), _table(tb, ctx.device)
    inst_a.paint_spans(zang.Span(0, F), [img_a], None, SR, trem, vib, table, split=True)
    inst_z.paint_spans(zang.Span(0, F), [img_z], None, SR, trem, vib, table, zero_first=True, split=True)
    ctx.sync()
    assert_bitexact(from_image(img_a), fr.split_image(base, m, c, painted, add_m), "split, added")
    assert_bitexact(from_image(img_z), fr.split_image(np.zeros((2 * V, F), np.float32), m, c, painted, add_m), "split, zero_first")
    _assert_state(inst_a, state, "split"); _assert_state(inst_z, state, "split, zero_first")
    inst_a.close(); inst_z.close()


# ------------------------------------------------------------------ tables made on the device
IMPULSE_FRAMES = (0, 256, 700)     # few distinct frames: the helper's frame-sequential loop runs once per distinct sub-span


def _pushes(rng, n_inst, per_inst):
    """per buffer: (instrument, frame, note_id, record) arrays in push order, impulses at IMPULSE_FRAMES"""
    inst, frame, ids, rec = [], [], [], []
    for i in range(n_inst):
        k = int(rng.integers(0, per_inst + 1))
        fs = np.sort(rng.choice(len(IMPULSE_FRAMES), k))
        for f in fs:
            inst.append(i); frame.append(IMPULSE_FRAMES[f]); ids.append(int(rng.integers(1, 9)))
            rec.append((float(np.float32(rng.uniform(60.0, 1500.0))), 1 if rng.random() < 0.65 else 0, (0, 0, 0)))
    return np.array(inst, np.uint32), np.array(frame, np.uint32), np.array(ids, np.uint64), np.array(rec, fr.REC)


def test_tables_a_live_voice_bank_makes_from_pushed_impulses(ctx):
    """26 synths of polyphony 5: per buffer the pushes go through zh_voice_bank_schedule_live, and paint_spans reads the bank's own
    tables on the device; the helper walks the same tables, downloaded."""
    from zang_amd import bank, zang
    x = fc.inputs()
    rng = np.random.default_rng(fc.SEED + 3)
    live = bank.LiveVoiceBank(ctx, NI, GROUP, fr.REC, fr.ON_OFFSET, 8 * NI, rows=8)
    table = live.span_table(8, 0)
    inst = _instrument(ctx)
    ref = fr.FMRef(V, GROUP, fc.patches())
    trem, vib = to_image(x["trem"]), to_image(x["vib"])
    img = ctx.image(F, V)
    spans = 0
    for b in range(3):
        live.push(*_pushes(rng, NI, 6))
        live.schedule(F, 8)
        inst.paint_spans(zang.Span(0, F), [img], None, SR, trem, vib, table, zero_first=True)
        got = live.download(8)
        K = max(int(got["count"].max()), 1)
        tb = {"count": got["count"], "start": got["start"][:K], "end": got["end"][:K], "freq": got["words"][0][:K].view(np.float32),
              "note_on": got["note_on"][:K], "note_id_changed": got["note_id_changed"][:K]}
        m, c, painted, add_m = ref.paint_spans(0, F, SR, x["trem"], x["vib"], tb)
        spans += int(got["count"].sum())
        assert_bitexact(from_image(img), fr.add_spans_into(np.zeros((V, F), np.float32), m, c, painted, add_m), f"buffer {b}")
        _assert_state(inst, ref.state(), f"buffer {b}")
    assert live.overflows() == 0 and spans > V
    inst.close(); live.close()


def test_schedule_and_paint_recorded_once_replayed_three_times(ctx):
    """a song bank's schedule and the FM paint over its tables as one graph, against the same two calls made eagerly"""
    import torch
    import zang_amd
    from tests import voice_bank_cases as vb
    from zang_amd import bank, zang
    x = fc.inputs()
    offsets, rec, t, ids = vb.corpus(NI, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
    banks = [bank.VoiceBank(c, GROUP, rec, offsets, t, ids, vb.ON_OFFSET, rows=34) for c in (ctx, c2)]
    insts = [_instrument(ctx), None]
    from zang_amd import modules as mod
    insts[1] = mod.FMInstrument(V, c2, group=GROUP)
    insts[1].set_patches(np.array(fc.patches(), np.uint32))
    imgs = [ctx.image(F, V), c2.image(F, V)]
    lfos = [(to_image(x["trem"]), to_image(x["vib"])) for _ in range(2)]
    tables = [b.span_table(34, 0) for b in banks]
    span = zang.Span(0, F)
    ctx.sync(); c2.sync()

    def body(i):
        banks[i].schedule([F], vb.SR, 34)
        insts[i].paint_spans(span, [imgs[i]], None, SR, lfos[i][0], lfos[i][1], tables[i], zero_first=True)
    g = c2.capture(lambda: body(1))
    names = [k for k, _ in g.kernels()]
    assert any("k_fm_spans" in k for k in names) and "k_voice_bank_schedule" in names, names
    sound = False
    for b in range(3):
        body(0)
        g.launch()
        ctx.sync(); c2.sync()
        got = from_image(imgs[1])
        assert_bitexact(got, from_image(imgs[0]), f"replay {b}")
        assert insts[1].state().tobytes() == insts[0].state().tobytes(), b
        sound = sound or bool(np.abs(got).max() > 0.05)
    assert sound and banks[1].overflows() == 0
    g.close()
    for o in insts + banks:
        o.close()
    c2.close()
