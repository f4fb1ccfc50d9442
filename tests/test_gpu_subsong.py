"""GPU: the subsong stage (zh_subsong_*, k_subsong_schedule) behind a live voice bank of polyphony 1, against
tests/subsong_reference.py: after each of six consecutive buffers of scripted pushes the stage's table, counts, overflow counter and
per-player state are the model's, at every player count; a get_state / set_state round trip mid-sequence changes nothing; a state
set into a fresh stage goes on as the model does; what the stage and the melody kit refuse."""
import ctypes as C

import numpy as np
import pytest

from tests import subsong_cases as sc
from tests import subsong_reference as sr

pytestmark = pytest.mark.gpu


def _push(bank, case, b, N, dtype):
    """one buffer's pushes of every player, in push order per player"""
    for p in range(N):
        evs = sc.script(case, p)[b]
        if not evs:
            continue
        rec = np.zeros(len(evs), dtype)
        rec["freq"], rec["note_on"], rec["melody"] = [e[2] for e in evs], [int(e[3]) for e in evs], [e[4] for e in evs]
        bank.push(np.full(len(evs), p, np.uint32), [e[0] for e in evs], [e[1] for e in evs], rec)


@pytest.fixture(scope="module")
def kit(ctx):
    from zang_amd import subsong
    k = subsong.MelodyKit(ctx, sc.KIT)
    yield k
    k.close()


def _make(ctx, kit, case, N):
    from zang_amd import subsong
    from zang_amd.bank import LiveVoiceBank
    bank = LiveVoiceBank(ctx, N, 1, subsong.KEY_PARAMS, subsong.KEY_PARAMS.fields["note_on"][1], 33 * N, rows=sc.OUTER_SPANS)
    stage = subsong.SubsongStage(ctx, N, kit, sc.BASE_FREQ, rows=case.max_spans)
    return bank, stage, subsong.key_table(bank, sc.OUTER_SPANS)


@pytest.mark.parametrize("N", sc.PLAYERS)
@pytest.mark.parametrize("case", sc.BANK_CASES, ids=sc.BANK_CASE_IDS)
def test_the_stage_equals_the_model_after_every_buffer(ctx, kit, case, N):
    from zang_amd import subsong
    rec = sc.run(case)
    bank, stage, outer = _make(ctx, kit, case, N)
    assert sc.state_words(stage.state()) == [sc.INIT_WORDS] * N                                   # create == init()
    dropped = 0
    for b in range(sc.BUFFERS):
        _push(bank, case, b, N, subsong.KEY_PARAMS)
        bank.schedule(sc.OUT_LEN, sc.OUTER_SPANS)
        stage.schedule(case.rate(b), sc.OUT_LEN, case.max_spans, outer)
        ctx.sync()
        assert ctx.last_form() == ["k_subsong_schedule"], ctx.last_form()
        got_outer = bank.download(sc.OUTER_SPANS)
        assert [int(c) for c in got_outer["count"]] == [len(o) for o in rec.outer[b][:N]], f"buffer {b}: the outer table"
        ref, d = sr.table(rec.inner[b][:N], case.max_spans)
        dropped += d
        got = stage.download(case.max_spans)
        assert sr.same_table(got, ref) is None, (f"buffer {b}", sr.same_table(got, ref))
        assert stage.overflows() == dropped, f"buffer {b}"
        assert sc.state_words(stage.state()) == rec.words[b][:N], f"buffer {b}: state"
        if b == 2:                                                   # a round trip mid-sequence changes nothing
            st = stage.state()
            stage.set_state(st)
            assert stage.state().tobytes() == st.tobytes()
    assert bank.overflows() == 0
    stage.close(); bank.close()


@pytest.mark.parametrize("name", ["key_change_carried_note", "more_than_32_events", "rate_nan"])
def test_a_set_state_is_where_the_model_goes_on_from(ctx, kit, name):
    """the state after buffer 1 of one run set into a FRESH stage (and the outer bank's state into a fresh bank): buffers 2-5 are
    the model's"""
    from zang_amd import subsong
    case, N = sc.case(name), 65
    rec = sc.run(case)
    bank, stage, outer = _make(ctx, kit, case, N)
    for b in range(2):
        _push(bank, case, b, N, subsong.KEY_PARAMS)
        bank.schedule(sc.OUT_LEN, sc.OUTER_SPANS)
    bank2, stage2, outer2 = _make(ctx, kit, case, N)
    bank2.set_state(bank.get_state())
    stage2.set_state(sc.state_array(rec.words[1][:N], stage2.state().dtype))
    assert sc.state_words(stage2.state()) == rec.words[1][:N]
    for b in range(2, sc.BUFFERS):
        _push(bank2, case, b, N, subsong.KEY_PARAMS)
        bank2.schedule(sc.OUT_LEN, sc.OUTER_SPANS)
        stage2.schedule(case.rate(b), sc.OUT_LEN, case.max_spans, outer2)
        ctx.sync()
        ref, _ = sr.table(rec.inner[b][:N], case.max_spans)
        got = stage2.download(case.max_spans)
        assert sr.same_table(got, ref) is None, (f"buffer {b}", sr.same_table(got, ref))
        assert sc.state_words(stage2.state()) == rec.words[b][:N], f"buffer {b}: state"
    for o in (stage, stage2, bank, bank2):
        o.close()


def _outer_on_device(outer, K):
    """a hand-made outer table [span][player] on the device, as a bank's views would hand it over: -> (zh_script_span_table, the
    three zh_script_span_param, what keeps the memory alive)"""
    from zang_amd import abi
    from tests import util
    N = len(outer)
    count = np.array([len(o) for o in outer], np.uint32)
    start, end, on, mel = (np.zeros((K, N), np.uint32) for _ in range(4))
    nic, freq = np.zeros((K, N), np.uint8), np.zeros((K, N), np.float32)
    for p, rows in enumerate(outer):
        for k, (s, e, (f, note_on, melody), changed) in enumerate(rows):
            start[k, p], end[k, p], nic[k, p], freq[k, p], on[k, p], mel[k, p] = s, e, changed, f, note_on, melody
    keep = [util.dev(a.view(np.int32) if a.dtype == np.uint32 else a) for a in (count, start, end, nic, freq, on, mel)]
    ptr = [t.data_ptr() for t in keep]
    tb = abi.ScriptSpanTable(K, 0, ptr[0], ptr[1], ptr[2], ptr[3])
    sp = (abi.ScriptSpanParam * abi.SUBSONG_IN_FIELDS)(abi.ScriptSpanParam(ptr[4], None), abi.ScriptSpanParam(None, ptr[5]), abi.ScriptSpanParam(None, ptr[6]))
    return tb, sp, keep


@pytest.mark.parametrize("case", [c for c in sc.CASES if not c.bank], ids=[c.name for c in sc.CASES if not c.bank])
def test_an_outer_table_no_bank_makes(ctx, kit, case):
    """an outer note-off with no earlier note-on (a voice bank's dispatcher would drop it): the model's outer sub-spans uploaded as
    a table of the caller's, the kernel's rows and state after every buffer are the model's"""
    import ctypes as C
    from zang_amd import abi, subsong
    N, K = 65, 4
    rec = sc.run(case)
    stage = subsong.SubsongStage(ctx, N, kit, sc.BASE_FREQ, rows=case.max_spans)
    assert not rec.outer[0][0][0][2][1] and rec.outer[0][0][0][0] > 0                 # buffer 0 opens with a gap, then a note-off
    for b in range(sc.BUFFERS):
        tb, sp, keep = _outer_on_device(rec.outer[b][:N], K)
        abi.check(ctx.lib.zh_subsong_schedule(stage.handle, case.rate(b), sc.OUT_LEN, case.max_spans, C.byref(tb), sp), "zh_subsong_schedule")
        ctx.sync()
        ref, dropped = sr.table(rec.inner[b][:N], case.max_spans)
        got = stage.download(case.max_spans)
        assert dropped == 0 and sr.same_table(got, ref) is None, (f"buffer {b}", sr.same_table(got, ref))
        assert sc.state_words(stage.state()) == rec.words[b][:N], f"buffer {b}: state"
        del keep
    assert any(rec.inner[0][p] for p in range(N))                                     # melody 0 did play under the note-off
    stage.close()


def test_reset_is_init_and_reserve_changes_the_capacity(ctx, kit):
    from zang_amd import abi, subsong
    case, N = sc.case("reference_melody_held"), 3
    rec = sc.run(case)
    bank, stage, outer = _make(ctx, kit, case, N)
    _push(bank, case, 0, N, subsong.KEY_PARAMS)
    bank.schedule(sc.OUT_LEN, sc.OUTER_SPANS)
    stage.schedule(case.rate(0), sc.OUT_LEN, case.max_spans, outer)
    assert sc.state_words(stage.state()) == rec.words[0][:N] != [sc.INIT_WORDS] * N
    stage.reset()
    assert sc.state_words(stage.state()) == [sc.INIT_WORDS] * N
    fresh = subsong.SubsongStage(ctx, N, kit, sc.BASE_FREQ)                                        # the capacity at creation: 33 rows
    assert fresh._schedule(sc.RATE, sc.OUT_LEN, 33, outer) == 0 and fresh._schedule(sc.RATE, sc.OUT_LEN, 34, outer) == abi.ZH_ERR_INVALID
    fresh.reserve(40)
    assert fresh._schedule(sc.RATE, sc.OUT_LEN, 40, outer) == 0
    empty = subsong.MelodyKit(ctx, [])                                                             # K = 0: no melody to latch
    none = subsong.SubsongStage(ctx, N, empty, sc.BASE_FREQ)
    assert [w[2] for w in sc.state_words(none.state())] == [sr.NO_MELODY] * N
    none.set_state(none.state())
    for o in (none, empty, fresh, stage, bank):
        o.close()


def test_refusals(ctx, kit):
    from zang_amd import abi, subsong
    case, N = sc.case("reference_melody_held"), 5
    bank, stage, outer = _make(ctx, kit, case, N)
    before = stage.state().tobytes()
    lib = ctx.lib
    assert stage._schedule(sc.RATE, sc.OUT_LEN, 0, outer) == abi.ZH_ERR_INVALID
    assert stage._schedule(sc.RATE, sc.OUT_LEN, case.max_spans + 1, outer) == abi.ZH_ERR_INVALID                 # above the capacity
    sp = (abi.ScriptSpanParam * abi.SUBSONG_IN_FIELDS)(outer.arrays["freq"], outer.arrays["note_on"], outer.arrays["melody"])
    assert lib.zh_subsong_schedule(None, sc.RATE, sc.OUT_LEN, 4, C.byref(outer.tb), sp) == abi.ZH_ERR_INVALID
    assert lib.zh_subsong_schedule(stage.handle, sc.RATE, sc.OUT_LEN, 4, None, sp) == abi.ZH_ERR_INVALID
    assert lib.zh_subsong_schedule(stage.handle, sc.RATE, sc.OUT_LEN, 4, C.byref(outer.tb), None) == abi.ZH_ERR_INVALID
    for missing in range(abi.SUBSONG_IN_FIELDS):                                                 # a NULL array in the params
        part = (abi.ScriptSpanParam * abi.SUBSONG_IN_FIELDS)(*[abi.ScriptSpanParam() if i == missing else sp[i] for i in range(3)])
        assert lib.zh_subsong_schedule(stage.handle, sc.RATE, sc.OUT_LEN, 4, C.byref(outer.tb), part) == abi.ZH_ERR_INVALID
    wrong = (abi.ScriptSpanParam * abi.SUBSONG_IN_FIELDS)(abi.ScriptSpanParam(None, outer.arrays["note_on"].u), sp[1], sp[2])
    assert lib.zh_subsong_schedule(stage.handle, sc.RATE, sc.OUT_LEN, 4, C.byref(outer.tb), wrong) == abi.ZH_ERR_INVALID   # freq as `u`
    t = outer.tb
    for tb in (abi.ScriptSpanTable(0, 0, t.count, t.start, t.end, t.note_id_changed), abi.ScriptSpanTable(t.max_spans, 0, None, t.start, t.end, t.note_id_changed),
               abi.ScriptSpanTable(t.max_spans, 0, t.count, None, t.end, t.note_id_changed), abi.ScriptSpanTable(t.max_spans, 0, t.count, t.start, None, t.note_id_changed),
               abi.ScriptSpanTable(t.max_spans, 0, t.count, t.start, t.end, None)):
        assert lib.zh_subsong_schedule(stage.handle, sc.RATE, sc.OUT_LEN, 4, C.byref(tb), sp) == abi.ZH_ERR_INVALID
    h = C.c_void_p()
    assert lib.zh_subsong_create(ctx.handle, 1, kit.handle, float("nan"), C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_subsong_create(ctx.handle, 1, None, 1.0, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_subsong_create(None, 1, kit.handle, 1.0, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_subsong_create(ctx.handle, 1, kit.handle, 1.0, None) == abi.ZH_ERR_INVALID
    one = abi.ScriptSpanParam()
    assert lib.zh_subsong_span_param(stage.handle, abi.SUBSONG_SPAN_FIELDS, C.byref(one)) == abi.ZH_ERR_INVALID
    tb = abi.ScriptSpanTable()
    assert lib.zh_subsong_script_table(stage.handle, case.max_spans + 1, C.byref(tb)) == abi.ZH_ERR_INVALID
    assert lib.zh_subsong_reserve(stage.handle, 0) == abi.ZH_ERR_INVALID
    st = stage.state()
    for bad in (sc.K, sc.K + 1, 0xfffffffe):                         # the melody indexes the kit
        st2 = st.copy()
        st2["melody"][N - 1] = bad
        assert lib.zh_subsong_set_state(stage.handle, st2.ctypes.data) == abi.ZH_ERR_INVALID
    st2 = st.copy()
    st2["melody"][:] = sr.NO_MELODY
    assert lib.zh_subsong_set_state(stage.handle, st2.ctypes.data) == 0
    stage.set_state(st)
    ctx.sync()
    assert stage.state().tobytes() == before and stage.overflows() == 0
    stage.close(); bank.close()


def _kit_rc(ctx, offsets, events):
    from zang_amd import abi
    off = np.asarray(offsets, np.uint32)
    ev = np.zeros(max(len(events), 1), np.dtype(abi.MelodyEvent))
    for i, (t, note_id) in enumerate(events):
        ev["t"][i], ev["note_id"][i], ev["freq"][i], ev["note_on"][i] = t, note_id, 220.0, 1
    h = C.c_void_p()
    rc = ctx.lib.zh_melody_kit_create(ctx.handle, off.ctypes.data, len(off) - 1, ev.ctypes.data, len(events), C.byref(h))
    if rc == 0:
        k, e = C.c_uint32(), C.c_uint32()
        assert ctx.lib.zh_melody_kit_count(h, C.byref(k), C.byref(e)) == 0 and (k.value, e.value) == (len(off) - 1, len(events))
        ctx.lib.zh_melody_kit_destroy(h)
    return rc


def test_what_a_melody_kit_refuses(ctx):
    from zang_amd import abi
    ev = [(0.0, 1), (0.1, 2), (0.1, 3), (0.05, 4), (0.2, 5)]         # the fourth starts a new melody: its t may be lower
    assert _kit_rc(ctx, [0, 3, 5], ev) == 0
    assert _kit_rc(ctx, [0], []) == 0                                # K = 0
    assert _kit_rc(ctx, [0, 0, 0, 5, 5], [(0.0, 1)] * 5) == 0        # empty melodies, equal times
    assert _kit_rc(ctx, [2, 3], ev) == 0                             # a kit may leave events out
    bad = abi.ZH_ERR_INVALID
    assert _kit_rc(ctx, [0, 4, 5], ev) == bad                        # t decreases inside a melody
    assert _kit_rc(ctx, [0, 2], [(0.0, 1), (float("nan"), 2)]) == bad
    assert _kit_rc(ctx, [0, 2], [(-0.5, 1), (0.0, 2)]) == bad
    assert _kit_rc(ctx, [0, 2], [(0.0, 1), (float("-inf"), 2)]) == bad
    assert _kit_rc(ctx, [0, 3, 2, 5], ev) == bad                     # offsets decrease
    assert _kit_rc(ctx, [0, 3, 6], ev) == bad                        # an offset past the events
    assert _kit_rc(ctx, [6, 6], ev) == bad
    h = C.c_void_p()
    off = np.zeros(2, np.uint32)
    evs = np.zeros(1, np.dtype(abi.MelodyEvent))
    assert ctx.lib.zh_melody_kit_create(None, off.ctypes.data, 1, evs.ctypes.data, 0, C.byref(h)) == bad
    assert ctx.lib.zh_melody_kit_create(ctx.handle, None, 1, evs.ctypes.data, 0, C.byref(h)) == bad
    assert ctx.lib.zh_melody_kit_create(ctx.handle, off.ctypes.data, 1, evs.ctypes.data, 0, None) == bad
    off[1] = 1
    assert ctx.lib.zh_melody_kit_create(ctx.handle, off.ctypes.data, 1, None, 1, C.byref(h)) == bad
    assert ctx.lib.zh_melody_kit_destroy(None) == bad and ctx.lib.zh_melody_kit_count(None, None, None) == bad
