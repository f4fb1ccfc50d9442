"""The edge rules of the Trigger sub-span walk, pinned on every walker: the tables of tests/span_walk_cases.py -- malformed
entries, empty sub-spans, sub-spans at and past the buffer's edges, lengths around the 8-frame chunk and the 64-frame block,
count > max_spans -- through NiceInstrument and PMOscInstrument (one wave per voice at 3 voices, one lane per voice at 65),
a builtin module's span paint (Envelope), FMInstrument and a generated script module (Pluck), all at 65 voices.

The expected image is one oracle paint per call of the model (span_walk_cases.trigger_calls), bit for bit, added onto a live
image and with zero_first.  The state is compared for the voices whose every reached sub-span ended: the oracle's paint always
runs the epilogue, the kernels skip it for a sub-span that runs into the buffer's end."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import span_walk_cases as sw
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
F, S, E = sw.IMG_F, sw.BUF_START, sw.BUF_END
gpu = pytest.mark.gpu


def test_the_model_on_the_cases():
    """trigger_calls against the calls each case's rule prescribes, written out by hand"""
    want = {0: [(0, 8, 40, True), (1, 40, 72, True), (2, 72, 104, True)], 1: [(0, 8, 104, True)],
            2: [(0, 10, 11, True), (1, 20, 27, True), (2, 30, 38, True)], 3: [(0, 9, 18, True), (1, 21, 84, True)],
            4: [(0, 13, 77, True)], 5: [(0, 11, 76, True)], 6: [(0, 50, 50, True), (1, 50, 70, True)],
            7: [(0, 20, 30, True), (1, 104, 104, True)], 8: [(0, 104, 104, False)], 9: [], 10: [(0, 10, 30, True)],
            11: [(0, 40, 104, False)], 12: [(0, 40, 104, False)], 13: [(0, 10, 20, True)],
            14: [(0, 8, 20, True), (1, 20, 30, True), (2, 40, 50, True)], 15: []}
    tb = sw.tables(len(sw.CASES))
    assert len(want) == len(sw.CASES)
    for v in range(len(sw.CASES)):
        assert sw.calls(tb, v) == want[v], sw.CASES[v][0]
    for V, offsets in sw.OFFSETS_FOR.items():                         # every case is reached at each voice count
        assert {(o + v) % len(sw.CASES) for o in offsets for v in range(V)} == set(range(len(sw.CASES)))
    assert tb["count"][14] == sw.ROWS > sw.K and tb["start"].shape[0] == sw.ROWS
    assert all(any(tb["note_id_changed"][k, v] for k in range(min(len(sw.CASES[v][1]), sw.K))) for v in range(len(sw.CASES)) if sw.CASES[v][1])


def _base(seed, V, zf):
    """(what the image holds before the paint, what it holds after a paint that adds nothing)"""
    base = util.rng_buffers(seed, V, F)
    ref = base.copy()
    if zf:
        ref[:, S:E] = 0.0
    return base, ref


def _span_table(tb, device):
    from zang_amd.spans import SpanTable
    t = SpanTable.from_arrays(tb["count"], tb["start"], tb["end"], tb["freq"], tb["note_on"], tb["note_id_changed"], device)
    assert t.c.max_spans == sw.ROWS
    t.c.max_spans = sw.K                                             # the arrays hold one row more than the kernel may read
    return t


def _assert_rows(gpu_rows, ref_rows, keep, what):
    util.assert_bitexact(np.asarray(gpu_rows)[keep], np.asarray(ref_rows)[keep], what)


@gpu
@pytest.mark.parametrize("zf", [True, False])
@pytest.mark.parametrize("V,form", [(3, "k_nice_spans_wave"), (65, "k_nice_spans")])
def test_nice_instrument(ctx, oracle, V, form, zf):
    from zang_amd import modules as mod, workloads, zang
    L = oracle.lib()
    _, color, _, _ = workloads.voice_params(4, 0, V)
    t0, t1 = np.zeros(F, np.float32), np.zeros(F, np.float32)
    for offset in sw.OFFSETS_FOR[V]:
        tb = sw.tables(V, offset)
        st = [oracle.NiceInstrument() for _ in range(V)]
        base, ref = _base(31 + offset, V, zf)
        for v in range(V):
            L.zo_nice_init(C.byref(st[v]), float(color[v]))
            for (k, s, e, _) in sw.calls(tb, v):
                L.zo_nice_paint(C.byref(st[v]), s, e, oracle.fptr(ref[v]), oracle.fptr(t0), oracle.fptr(t1), int(tb["note_id_changed"][k, v]),
                                SR, float(tb["freq"][k, v]), int(tb["note_on"][k, v]))
        m = mod.NiceInstrument(V, util.dev(color), ctx)
        out = util.to_image(base)
        m.paint_spans(zang.Span(S, E), [out], None, SR, _span_table(tb, ctx.device), zero_first=zf)
        ctx.sync()
        assert ctx.last_form() == [form], ctx.last_form()
        util.assert_bitexact(util.from_image(out), ref, f"nice V={V} offset {offset} zf={zf}")
        gs, keep = m.state(), sw.all_ended(tb, V)
        _assert_rows(gs["osc"]["cnt"].astype(np.uint32), np.array([r.osc.cnt for r in st], np.uint32), keep, "cnt")
        _assert_rows(gs["flt"]["l"].astype(np.float32), np.array([r.flt.l for r in st], np.float32), keep, "l")
        _assert_rows(gs["flt"]["b"].astype(np.float32), np.array([r.flt.b for r in st], np.float32), keep, "b")
        _assert_rows(gs["env"]["state"].astype(np.uint32), np.array([r.env.state for r in st], np.uint32), keep, "env.state")
        _assert_rows(gs["env"]["t"].astype(np.float32), np.array([r.env.painter.t for r in st], np.float32), keep, "env.t")
        _assert_rows(gs["env"]["last_value"].astype(np.float32), np.array([r.env.painter.last_value for r in st], np.float32), keep, "env.last_value")
        m.close()


@gpu
@pytest.mark.parametrize("zf", [True, False])
@pytest.mark.parametrize("V,form", [(3, "k_pmosc_spans_wave"), (65, "k_pmosc_spans")])
def test_pmosc_instrument(ctx, oracle, V, form, zf):
    from zang_amd import modules as mod, zang
    L = oracle.lib()
    rel = np.random.default_rng(3).uniform(0.05, 0.5, V).astype(np.float32)
    t0, t1, t2 = np.zeros(F, np.float32), np.zeros(F, np.float32), np.zeros(F, np.float32)
    for offset in sw.OFFSETS_FOR[V]:
        tb = sw.tables(V, offset)
        st = [oracle.PMOscInstrument() for _ in range(V)]
        base, ref = _base(47 + offset, V, zf)
        for v in range(V):
            L.zo_pmosc_init(C.byref(st[v]), float(rel[v]))
            for (k, s, e, _) in sw.calls(tb, v):
                L.zo_pmosc_paint(C.byref(st[v]), s, e, oracle.fptr(ref[v]), oracle.fptr(t0), oracle.fptr(t1), oracle.fptr(t2),
                                 int(tb["note_id_changed"][k, v]), SR, float(tb["freq"][k, v]), int(tb["note_on"][k, v]))
        m = mod.PMOscInstrument(V, util.dev(rel), ctx)
        out = util.to_image(base)
        m.paint_spans(zang.Span(S, E), [out], None, SR, _span_table(tb, ctx.device), zero_first=zf)
        ctx.sync()
        assert ctx.last_form() == [form], ctx.last_form()
        util.assert_bitexact(util.from_image(out), ref, f"pmosc V={V} offset {offset} zf={zf}")
        gs, keep = m.state(), sw.all_ended(tb, V)
        _assert_rows(gs["carrier"]["t"].astype(np.float32), np.array([r.carrier.t for r in st], np.float32), keep, "carrier.t")
        _assert_rows(gs["modulator"]["t"].astype(np.float32), np.array([r.modulator.t for r in st], np.float32), keep, "modulator.t")
        _assert_rows(gs["env"]["state"].astype(np.uint32), np.array([r.env.state for r in st], np.uint32), keep, "env.state")
        _assert_rows(gs["env"]["t"].astype(np.float32), np.array([r.env.painter.t for r in st], np.float32), keep, "env.t")
        m.close()


@gpu
@pytest.mark.parametrize("zf", [True, False])
def test_builtin_module_spans(ctx, oracle, zf):
    """Envelope through module_spans: note_id_changed matters to its prologue, and its epilogue keeps the painter's clock"""
    from tests.module_spans_cases import CASES, _defaults
    from zang_amd import zang
    V = 65
    case = CASES["envelope"]()
    rng = np.random.default_rng(5)
    L = oracle.lib()
    tb = sw.tables(V)
    case.dflt = _defaults(case, rng, V)
    case.arr = {name: gen(rng, (sw.ROWS, V)) for name, gen in case.fields}
    sts = [case.oracle_init(oracle, L) for _ in range(V)]
    base, ref = _base(59, V, zf)
    for v in range(V):
        for (k, s, e, _) in sw.calls(tb, v):
            case.oracle_paint(oracle, L, sts[v], v, s, e, ref[v], int(tb["note_id_changed"][k, v]), k, {})
    m = case.make(ctx, V)
    out = util.to_image(base)
    table = m.span_table(tb["count"], tb["start"], tb["end"], tb["note_id_changed"], case.arr)
    table.max_spans = sw.K                                           # (read when the table goes to the device: the arrays keep ROWS rows)
    m.paint_spans(zang.Span(S, E), [out], None, case.params(m, case.dflt, {}), table, zero_first=zf)
    ctx.sync()
    assert ctx.last_form() == ["k_envelope_spans"], ctx.last_form()
    util.assert_bitexact(util.from_image(out), ref, f"envelope zf={zf}")
    keep = sw.all_ended(tb, V)
    for i, (got, want) in enumerate(case.state(m, sts)):
        _assert_rows(got, want, keep, f"envelope state {i}")
    m.close()


@gpu
@pytest.mark.parametrize("zf", [True, False])
def test_fm_instrument(ctx, zf):
    """k_fm_spans against the helper's Instrument.paint, one call per call of the model (voices that make the same call together)"""
    from tests import fm_cases as fc, fm_reference as fr
    from zang_amd import modules as mod, zang
    V, GROUP = 65, 5
    NI = V // GROUP
    patches = fc.patches()[:NI]
    rng = np.random.default_rng(71)
    trem = rng.uniform(-1.0, 1.0, (NI, F)).astype(np.float32)
    vib = rng.uniform(-1.0, 1.0, (NI, F)).astype(np.float32)
    tb = sw.tables(V)
    ref = fr.FMRef(V, GROUP, patches)
    m_add, c_add = np.zeros((V, F), np.float32), np.zeros((V, F), np.float32)
    painted = np.zeros((V, F), bool)
    groups = {}
    for v in range(V):
        for (k, s, e, _) in sw.calls(tb, v):
            groups.setdefault((k, s, e), []).append(v)
    for (k, s, e), vs in sorted(groups.items()):                     # ascending k: every voice's calls in its own order
        vs = np.array(vs)
        mm, cc, _ = ref.paint(s, e, tb["note_id_changed"][k, vs] != 0, SR, trem, vib, tb["freq"][k, vs], tb["note_on"][k, vs] != 0, vs)
        m_add[vs, s:e], c_add[vs, s:e], painted[vs, s:e] = mm, cc, True
    base, want = _base(83, V, zf)
    want = fr.add_spans_into(want, m_add, c_add, painted, ref.alg == 0)
    inst = mod.FMInstrument(V, ctx, group=GROUP)
    inst.set_patches(np.array(patches, np.uint32))
    out = util.to_image(base)
    inst.paint_spans(zang.Span(S, E), [out], None, SR, util.to_image(trem), util.to_image(vib), _span_table(tb, ctx.device), zero_first=zf)
    ctx.sync()
    assert any("k_fm_spans" in name for name in ctx.last_form()), ctx.last_form()
    util.assert_bitexact(util.from_image(out), want, f"fm zf={zf}")
    got = np.frombuffer(inst.state().tobytes(), fr.STATE_DTYPE).reshape(V, 2)
    keep, st = sw.all_ended(tb, V), ref.state()
    for name in fr.STATE_DTYPE.names:
        _assert_rows(got[name], st[name], keep, f"fm state.{name}")
    inst.close()


@gpu
@pytest.mark.parametrize("zf", [True, False])
def test_generated_module_spans(ctx, zf):
    """Pluck (a SineOsc, whose epilogue wraps its phase, times an Envelope, whose prologue reads note_id_changed) in its spans form
    against the interpreter; then one plain paint of the whole image, which must go on from the state the spans left"""
    from oracle import zangscript as zs
    from oracle import zs_interp
    from zang_amd import script, zang
    V, name = 65, "Pluck"
    path = os.path.join(ROOT, "tests", "golden", "script_modules.txt")
    text = open(path).read()
    prog = script.ScriptProgram(text, ctx, filename=os.path.basename(path), only=[name], spans=True)
    try:
        m = prog.module(name, V)
        assert [n for n, _, _ in m.params] == ["sample_rate", "freq", "note_on"], m.params
        s_ = zs.compile(text, os.path.basename(path))
        interp = [zs_interp.Instance(s_, s_.module_index(name), iter(())) for _ in range(V)]
        tb = sw.tables(V)
        base, ref = _base(97, V, zf)
        for v in range(V):
            for (k, s, e, _) in sw.calls(tb, v):
                interp[v].paint(s, e, ref[v], bool(tb["note_id_changed"][k, v]), [np.float32(SR), np.float32(tb["freq"][k, v]), bool(tb["note_on"][k, v])])
        table = script.ScriptSpanTable(m.params, tb["count"], tb["start"], tb["end"], tb["note_id_changed"],
                                       {"freq": (tb["freq"], None), "note_on": (None, tb["note_on"].astype(np.uint32))})
        table.max_spans = sw.K                                       # (read when the table goes to the device: the arrays keep ROWS rows)
        out = util.to_image(base)
        m.paint_spans(zang.Span(S, E), [out], table, {"sample_rate": SR}, zero_first=zf)
        ctx.sync()
        assert ctx.last_form() == ["zs_paint_spans_" + name], ctx.last_form()
        util.assert_bitexact(util.from_image(out), ref, f"{name} zf={zf}")
        keep = sw.all_ended(tb, V)
        after = np.zeros((V, F), np.float32)
        for v in np.nonzero(keep)[0]:
            interp[v].paint(0, F, after[v], False, [np.float32(SR), np.float32(330.0), False])
        out2 = ctx.image(F, V, fill=5.0)
        m.paint(zang.Span(0, F), [out2], None, False, {"sample_rate": SR, "freq": 330.0, "note_on": False}, zero_first=True)
        ctx.sync()
        _assert_rows(util.from_image(out2), after, keep, f"{name}: a plain paint after the spans")
    finally:
        prog.close()
