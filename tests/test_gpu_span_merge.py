"""GPU: the merge stage (zh_span_merge_*, k_span_merge) through the C ABI against tests/two_reference.py: the case list of
tests/two_cases.py (the hand-written tables first, then random ones) uploaded as two source tables, for 1, 63, 64, 65 and 130
players and both field shapes -- rows, counts and the overflow counter are the model's; reserve, every refusal, n = 0, and a
captured-and-replayed schedule against a direct one."""
import ctypes as C

import numpy as np
import pytest

from tests import two_cases as tc
from tests import two_reference as tr

pytestmark = pytest.mark.gpu
PLAYERS = [1, 63, 64, 65, 130]


class DevSource:
    """a source table on the device: .tb (zh_script_span_table) and .fields (zh_script_span_param per field, of its kind)"""

    def __init__(self, players_rows, kinds, spans=tc.SOURCE_SPANS):
        import torch
        from zang_amd import abi
        self.kinds, self.spans = kinds, spans
        host = tr.source_table(players_rows, len(kinds), spans, filler_end=tc.OUT_LEN)
        n = max(len(players_rows), 1)                                  # n = 0: one-element blocks, so that no pointer is NULL
        self.dev = {}
        for k, a in host.items():
            flat = np.zeros(max(a.size, n), a.dtype)
            flat[:a.size] = a.reshape(-1)
            self.dev[k] = torch.from_numpy(flat.view(np.int32) if a.dtype == np.uint32 else flat).cuda()
        d = self.dev
        self.tb = abi.ScriptSpanTable(spans, 0, d["count"].data_ptr(), d["start"].data_ptr(), d["end"].data_ptr(), d["nic"].data_ptr())
        plane = spans * len(players_rows) * 4
        self.fields = (abi.ScriptSpanParam * len(kinds))()
        for f, kind in enumerate(kinds):
            ptr = d["words"].data_ptr() + f * plane
            self.fields[f] = abi.ScriptSpanParam(ptr, None) if kind == "f" else abi.ScriptSpanParam(None, ptr)

    def refill(self, players_rows):
        """other rows into the same device blocks"""
        import torch
        host = tr.source_table(players_rows, len(self.kinds), self.spans, filler_end=tc.OUT_LEN)
        for k, a in host.items():
            flat = a.reshape(-1)
            self.dev[k][:flat.size].copy_(torch.from_numpy(flat.view(np.int32) if a.dtype == np.uint32 else flat))


def _stage(ctx, n, shape, rows=None):
    from zang_amd import two
    fa = [(f"a{i}", k) for i, k in enumerate(shape.kinds_a)]
    fb = [(f"b{i}", k) for i, k in enumerate(shape.kinds_b)]
    return two.SpanMerge(ctx, n, fa, f"a{shape.on_a}", fb, f"b{shape.on_b}", rows=rows)


def _schedule(stage, a, b, out_len, max_spans):
    return stage.lib.zh_span_merge_schedule(stage.handle, out_len, max_spans, C.byref(a.tb), a.fields, C.byref(b.tb), b.fields)


def _download(stage, max_spans):
    got = stage.download(max_spans)
    got["words"] = np.stack([got[name] for name in stage.names])
    return got


def _model(pa, pb, shape, max_spans):
    return tr.merge_table(pa, shape.on_a, pb, shape.on_b, tc.OUT_LEN, max_spans, len(shape.kinds_a) + len(shape.kinds_b) + 3)


@pytest.mark.parametrize("N", PLAYERS)
@pytest.mark.parametrize("shape", [tc.EXAMPLE, tc.WIDE], ids=["example", "wide"])
def test_the_stage_equals_the_model(ctx, shape, N):
    pa, pb = tc.players(N, shape)
    stage = _stage(ctx, N, shape)
    a, b = DevSource(pa, shape.kinds_a), DevSource(pb, shape.kinds_b)
    assert _schedule(stage, a, b, tc.OUT_LEN, tc.MAX_SPANS) == 0
    ctx.sync()
    assert ctx.last_form() == ["k_span_merge"], ctx.last_form()
    ref, dropped = _model(pa, pb, shape, tc.MAX_SPANS)
    got = _download(stage, tc.MAX_SPANS)
    assert dropped == 0 and tr.same_table(got, ref) is None, tr.same_table(got, ref)
    assert stage.overflows() == 0
    if N >= len(tc.HAND) and shape == tc.EXAMPLE:                      # the hand-written rows, straight from the device
        for p, case in enumerate(tc.HAND):
            rows = [(int(got["start"][k, p]), int(got["end"][k, p]), int(got["nic"][k, p]), [int(x) for x in got["words"][:, k, p]])
                    for k in range(int(got["count"][p]))]
            assert rows == [(s, e, nic, list(w)) for s, e, nic, w in case.expect], case.name
    stage.close()


def test_the_views_kinds_and_named_fields(ctx):
    from zang_amd import abi
    stage = _stage(ctx, 3, tc.WIDE)
    t = stage.script_table(tc.MAX_SPANS)
    kinds = tc.WIDE.kinds_a + tc.WIDE.kinds_b + "uuu"
    for name, kind in zip(stage.names, kinds):
        sp = t.arrays[name]
        assert (sp.f is not None, sp.u is not None) == (kind == "f", kind == "u"), name
    base = len(tc.WIDE.kinds_a) + len(tc.WIDE.kinds_b)
    assert [stage.names[base + i] for i in (abi.SPAN_MERGE_NOTE_ON, abi.SPAN_MERGE_NIC_A, abi.SPAN_MERGE_NIC_B)] == ["note_on", "nic_a", "nic_b"]
    ptrs = [t.arrays[n].f or t.arrays[n].u for n in stage.names]
    assert [q - p for p, q in zip(ptrs, ptrs[1:])] == [tc.MAX_SPANS * 3 * 4] * (len(ptrs) - 1)      # [field][capacity rows][players]
    stage.close()


@pytest.mark.parametrize("max_spans", tc.OVERFLOW_MAX_SPANS)
def test_overflow_stops_the_list_and_counts_the_dropped_rows(ctx, max_spans):
    N = 130
    pa, pb = tc.players(N)
    stage = _stage(ctx, N, tc.EXAMPLE)
    a, b = DevSource(pa, "fu"), DevSource(pb, "fu")
    ref, dropped = _model(pa, pb, tc.EXAMPLE, max_spans)
    assert dropped > N
    for times in (1, 2):                                               # the counter adds up over schedules
        assert _schedule(stage, a, b, tc.OUT_LEN, max_spans) == 0
        assert stage.overflows() == times * dropped
    got = _download(stage, max_spans)
    assert tr.same_table(got, ref) is None, tr.same_table(got, ref)
    stage.close()


def test_reserve(ctx):
    from zang_amd import abi
    N = 65
    pa, pb = tc.players(N)
    stage = _stage(ctx, N, tc.EXAMPLE)
    a, b = DevSource(pa, "fu"), DevSource(pb, "fu")
    assert _schedule(stage, a, b, tc.OUT_LEN, tc.MAX_SPANS + 1) == abi.ZH_ERR_INVALID               # 67 rows at creation
    assert stage.lib.zh_span_merge_reserve(stage.handle, 0) == abi.ZH_ERR_INVALID
    stage.reserve(80)
    assert _schedule(stage, a, b, tc.OUT_LEN, 81) == abi.ZH_ERR_INVALID and _schedule(stage, a, b, tc.OUT_LEN, 80) == 0
    ref, _ = _model(pa, pb, tc.EXAMPLE, 80)
    got = _download(stage, 80)
    assert tr.same_table(got, ref) is None and stage.overflows() == 0
    stage.reserve(3)
    tb = abi.ScriptSpanTable()
    assert stage.lib.zh_span_merge_script_table(stage.handle, 4, C.byref(tb)) == abi.ZH_ERR_INVALID
    assert _schedule(stage, a, b, tc.OUT_LEN, 4) == abi.ZH_ERR_INVALID and _schedule(stage, a, b, tc.OUT_LEN, 3) == 0
    ref, dropped = _model(pa, pb, tc.EXAMPLE, 3)
    assert tr.same_table(_download(stage, 3), ref) is None and stage.overflows() == dropped > 0
    stage.reserve(3)                                                   # the same capacity: nothing happens
    assert tr.same_table(_download(stage, 3), ref) is None
    stage.close()


def test_no_players(ctx):
    stage = _stage(ctx, 0, tc.EXAMPLE)
    a, b = DevSource([], "fu"), DevSource([], "fu")
    assert _schedule(stage, a, b, tc.OUT_LEN, tc.MAX_SPANS) == 0
    ctx.sync()
    assert stage.overflows() == 0 and stage.download(tc.MAX_SPANS)["count"].shape == (0,)
    stage.close()


def test_refusals(ctx):
    from zang_amd import abi
    lib = ctx.lib
    N = 5
    pa, pb = tc.players(N)
    stage = _stage(ctx, N, tc.EXAMPLE)
    a, b = DevSource(pa, "fu"), DevSource(pb, "fu")
    sched = lambda ta, fa, tb, fb, max_spans=4: lib.zh_span_merge_schedule(stage.handle, tc.OUT_LEN, max_spans, ta, fa, tb, fb)
    ta, tb = C.byref(a.tb), C.byref(b.tb)
    assert sched(ta, a.fields, tb, b.fields) == 0
    ctx.sync()
    before = _download(stage, 4)
    # NULL arguments
    assert lib.zh_span_merge_schedule(None, tc.OUT_LEN, 4, ta, a.fields, tb, b.fields) == abi.ZH_ERR_INVALID
    for args in ((None, a.fields, tb, b.fields), (ta, None, tb, b.fields), (ta, a.fields, None, b.fields), (ta, a.fields, tb, None)):
        assert sched(*args) == abi.ZH_ERR_INVALID
    # a NULL array in either table, a table without rows
    for which in ("count", "start", "end", "note_id_changed"):                 # `start` is never read, and still may not be NULL
        for side in (0, 1):
            src = (a, b)[side].tb
            bad = abi.ScriptSpanTable(src.max_spans, 0, src.count, src.start, src.end, src.note_id_changed)
            setattr(bad, which, None)
            args = [ta, a.fields, tb, b.fields]
            args[2 * side] = C.byref(bad)
            assert sched(*args) == abi.ZH_ERR_INVALID, (which, side)
    norows = abi.ScriptSpanTable(0, 0, a.tb.count, a.tb.start, a.tb.end, a.tb.note_id_changed)
    assert sched(C.byref(norows), a.fields, tb, b.fields) == abi.ZH_ERR_INVALID
    # max_spans of 0 or above the capacity
    assert sched(ta, a.fields, tb, b.fields, 0) == abi.ZH_ERR_INVALID and sched(ta, a.fields, tb, b.fields, tc.MAX_SPANS + 1) == abi.ZH_ERR_INVALID
    # a field array of the wrong kind: `u` where the field is `f`, `f` where it is `u`, both, none
    for f, wrong in ((0, abi.ScriptSpanParam(None, a.fields[0].f)), (1, abi.ScriptSpanParam(a.fields[1].u, None)),
                     (0, abi.ScriptSpanParam(a.fields[0].f, a.fields[0].f)), (1, abi.ScriptSpanParam())):
        bad = (abi.ScriptSpanParam * 2)(a.fields[0], a.fields[1])
        bad[f] = wrong
        assert sched(ta, bad, tb, b.fields) == abi.ZH_ERR_INVALID and sched(ta, a.fields, tb, bad) == abi.ZH_ERR_INVALID, f
    # creation: n_fields outside 1..4, a kind that is neither, an on_field out of range or not `u`
    good = abi.SpanMergeSource(2, 1, (C.c_uint8 * 4)(ord("f"), ord("u"), 0, 0))
    h = C.c_void_p()
    create = lambda sa, sb: lib.zh_span_merge_create(ctx.handle, N, sa, sb, C.byref(h))
    for n_fields, on, kinds in ((0, 0, "uuuu"), (5, 0, "uuuu"), (2, 2, "uu"), (2, 0, "fu"), (2, 1, "ux"), (4, 3, "uuuf"), (1, 0, "f")):
        bad = abi.SpanMergeSource(n_fields, on, (C.c_uint8 * 4)(*[ord(k) for k in kinds.ljust(4, "\0")]))
        assert create(C.byref(bad), C.byref(good)) == abi.ZH_ERR_INVALID and create(C.byref(good), C.byref(bad)) == abi.ZH_ERR_INVALID, (n_fields, on, kinds)
    assert create(None, C.byref(good)) == abi.ZH_ERR_INVALID and create(C.byref(good), None) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_create(ctx.handle, N, C.byref(good), C.byref(good), None) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_create(None, N, C.byref(good), C.byref(good), C.byref(h)) == abi.ZH_ERR_INVALID
    # the views
    sp, out = abi.ScriptSpanParam(), abi.ScriptSpanTable()
    assert lib.zh_span_merge_span_param(stage.handle, 7, C.byref(sp)) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_span_param(stage.handle, 6, C.byref(sp)) == 0 and lib.zh_span_merge_span_param(stage.handle, 0, None) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_script_table(stage.handle, 0, C.byref(out)) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_script_table(stage.handle, tc.MAX_SPANS + 1, C.byref(out)) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_overflows(stage.handle, None) == abi.ZH_ERR_INVALID and lib.zh_span_merge_destroy(None) == abi.ZH_ERR_INVALID
    assert lib.zh_span_merge_reserve(None, 4) == abi.ZH_ERR_INVALID
    ctx.sync()
    assert tr.same_table(_download(stage, 4), before) is None            # a refused call wrote nothing
    stage.close()


def test_a_captured_schedule_replays_as_a_direct_one():
    """the capture records one kernel and runs nothing; each replay reads the sources as they are then.  On a side stream with a
    context of its own: the default stream cannot be captured"""
    import torch
    import zang_amd
    N = 65
    pa, pb = tc.players(N)
    with torch.cuda.stream(torch.cuda.Stream()):
        c2 = zang_amd.Context(0)
        direct, captured = _stage(c2, N, tc.EXAMPLE), _stage(c2, N, tc.EXAMPLE)
        a, b = DevSource(pa, "fu"), DevSource(pb, "fu")
        assert _schedule(direct, a, b, tc.OUT_LEN, tc.MAX_SPANS) == 0
        c2.sync()
        rc = []
        g = c2.capture(lambda: rc.append(_schedule(captured, a, b, tc.OUT_LEN, tc.MAX_SPANS)))
        assert rc == [0] and g.kernels() == [("k_span_merge", 1)], (rc, g.kernels())
        c2.sync()
        assert not captured.download(tc.MAX_SPANS)["count"].any()      # recorded, not run
        g.launch()
        c2.sync()
        want = _download(direct, tc.MAX_SPANS)
        assert tr.same_table(_download(captured, tc.MAX_SPANS), want) is None and int(want["count"].max()) > 40
        pa2, pb2 = tc.players(N, seed=7)
        pa2, pb2 = pa2[::-1], pb2[::-1]
        a.refill(pa2); b.refill(pb2)
        g.launch()
        assert _schedule(direct, a, b, tc.OUT_LEN, tc.MAX_SPANS) == 0
        c2.sync()
        ref, _ = _model(pa2, pb2, tc.EXAMPLE, tc.MAX_SPANS)
        got = _download(captured, tc.MAX_SPANS)
        assert tr.same_table(got, ref) is None and tr.same_table(_download(direct, tc.MAX_SPANS), ref) is None
        assert tr.same_table(got, want) is not None
        g.close()
        for o in (direct, captured):
            o.close()
        c2.close()
