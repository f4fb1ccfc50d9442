"""GPU: the key fan-out stage (zh_keyfan_*, k_keyfan_schedule) behind a live voice bank of polyphony 1, against
tests/polyphony_reference.py: after each of six consecutive buffers of scripted key events the stage's table (through both of its
views), counts, overflow counter and per-voice state are the model's, for 1 and 65 players of 1, 41 and 64 keys (65 x 41 lanes
cross several waves and end in a ragged one); a get_state / set_state round trip mid-sequence changes nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import polyphony_cases as pc
from tests import polyphony_reference as pr

pytestmark = pytest.mark.gpu
PLAYERS = [1, 65]
INIT = [1, 0, 0, 0, 0, 0]                                              # Voice :50-56: all zero, next_id = 1


def _push(bank, pushed, held_dtype):
    """one buffer's keyEvent pushes of every player, in push order per player"""
    for p, evs in enumerate(pushed):
        if not evs:
            continue
        rec = np.zeros(len(evs), held_dtype)
        rec["held_lo"] = [m & 0xffffffff for _, _, m in evs]
        rec["held_hi"] = [m >> 32 for _, _, m in evs]
        rec["on"] = 1
        bank.push(np.full(len(evs), p, np.uint32), [f for f, _, _ in evs], [i for _, i, _ in evs], rec)


def _make(ctx, case, N):
    from zang_amd import arp, polyphony
    from zang_amd.bank import LiveVoiceBank
    bank = LiveVoiceBank(ctx, N, 1, arp.HELD_PARAMS, arp.HELD_PARAMS.fields["on"][1], 33 * N, rows=pc.OUTER_SPANS)
    stage = polyphony.KeyFanStage(ctx, N, case.key_freqs(), rows=case.max_spans)
    return bank, stage, arp.held_table(bank, pc.OUTER_SPANS)


@pytest.mark.parametrize("N", PLAYERS)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_the_stage_equals_the_model_after_every_buffer(ctx, case, N):
    from zang_amd import arp
    rec = pc.run(case)
    V = N * case.n_keys
    bank, stage, outer = _make(ctx, case, N)
    assert pc.state_words(stage.state()) == [INIT] * V                                       # create == init()
    dropped = 0
    for b in range(pc.BUFFERS):
        _push(bank, rec.pushed[b][:N], arp.HELD_PARAMS)
        bank.schedule(pc.OUT_LEN, pc.OUTER_SPANS)
        stage.schedule(pc.OUT_LEN, case.max_spans, outer)
        ctx.sync()
        assert ctx.last_form() == ["k_keyfan_schedule"], ctx.last_form()
        got_outer = bank.download(pc.OUTER_SPANS)
        assert [int(c) for c in got_outer["count"]] == [len(o) for o in rec.outer[b][:N]], f"buffer {b}: the outer table"
        ref, d = pr.table(pc.voices_of(rec.inner[b], case, N), case.max_spans)
        dropped += d
        got = stage.download(case.max_spans)
        assert pr.same_table(got, ref) is None, (f"buffer {b}", pr.same_table(got, ref))
        ref8 = dict(ref, note_on=ref["note_on"].astype(np.uint8))                            # zh_keyfan_span_table's byte plane
        assert pr.same_table(dict(got, note_on=got["note_on8"]), ref8, names=("note_on",)) is None, f"buffer {b}: note_on as bytes"
        assert stage.overflows() == dropped, f"buffer {b}"
        assert pc.state_words(stage.state()) == pc.voices_of(rec.words[b], case, N), f"buffer {b}: state"
        if b == 2:                                                   # a round trip mid-sequence changes nothing
            st = stage.state()
            stage.set_state(st)
            assert stage.state().tobytes() == st.tobytes()
    assert (dropped > 0) == (case.name == "overflow") and bank.overflows() == 0
    stage.close(); bank.close()


def test_the_span_table_view_is_the_script_views_arrays(ctx):
    """zh_keyfan_span_table serves zh_span_table from the arrays zh_keyfan_script_table / _span_param hand out, plus the bytes"""
    from zang_amd import abi
    case, N = pc.CASES[0], 3
    bank, stage, outer = _make(ctx, case, N)
    t, s = stage.span_table(case.max_spans).c, stage.script_table(case.max_spans)
    assert (t.max_spans, t.count, t.start, t.end, t.note_id_changed) == (case.max_spans, s.tb.count, s.tb.start, s.tb.end, s.tb.note_id_changed)
    assert t.freq == s.arrays["freq"].f and not s.arrays["freq"].u
    assert s.arrays["note_on"].u and not s.arrays["note_on"].f and t.note_on and t.note_on != s.arrays["note_on"].u
    assert ctx.lib.zh_keyfan_span_table(stage.handle, case.max_spans + 1, C.byref(abi.SpanTable())) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_keyfan_span_table(stage.handle, 0, C.byref(abi.SpanTable())) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_keyfan_span_table(stage.handle, 1, None) == abi.ZH_ERR_INVALID
    stage.close(); bank.close()


def test_a_set_state_is_where_the_model_goes_on_from(ctx):
    """the state after buffer 2 of one run set into a FRESH stage (and the outer bank's state into a fresh bank): buffers 3-5 are
    the model's; any words round-trip (freq as bits: a NaN's payload too)"""
    from zang_amd import arp
    case, N = pc.CASES[0], 65
    rec = pc.run(case)
    bank, stage, outer = _make(ctx, case, N)
    for b in range(3):
        _push(bank, rec.pushed[b][:N], arp.HELD_PARAMS)
        bank.schedule(pc.OUT_LEN, pc.OUTER_SPANS)
    bank2, stage2, outer2 = _make(ctx, case, N)
    bank2.set_state(bank.get_state())
    stage2.set_state(pc.state_array(pc.voices_of(rec.words[2], case, N), stage2.state().dtype))
    for b in range(3, pc.BUFFERS):
        _push(bank2, rec.pushed[b][:N], arp.HELD_PARAMS)
        bank2.schedule(pc.OUT_LEN, pc.OUTER_SPANS)
        stage2.schedule(pc.OUT_LEN, case.max_spans, outer2)
        ctx.sync()
        ref, _ = pr.table(pc.voices_of(rec.inner[b], case, N), case.max_spans)
        got = stage2.download(case.max_spans)
        assert pr.same_table(got, ref) is None, (f"buffer {b}", pr.same_table(got, ref))
        assert pc.state_words(stage2.state()) == pc.voices_of(rec.words[b], case, N), f"buffer {b}: state"
    words = [[2 ** 64 - 1, 0xfffffffe, 7, 2 ** 63 + 5, 0x7fc12345, 0x80000000], [1, 2, 3, 4, 0xffffffff, 6]] * (N * case.n_keys // 2) + [INIT]
    stage.set_state(pc.state_array(words, stage.state().dtype))
    assert pc.state_words(stage.state()) == words
    stage.reset()
    assert pc.state_words(stage.state()) == [INIT] * (N * case.n_keys)
    for o in (stage, stage2, bank, bank2):
        o.close()


def test_refusals(ctx):
    from zang_amd import abi
    case, N = pc.CASES[0], 5
    bank, stage, outer = _make(ctx, case, N)
    before = stage.state().tobytes()
    lib, inv = ctx.lib, abi.ZH_ERR_INVALID
    assert stage._schedule(pc.OUT_LEN, 0, outer) == inv
    assert stage._schedule(pc.OUT_LEN, case.max_spans + 1, outer) == inv                      # above the capacity
    held = (abi.ScriptSpanParam * 2)(outer.arrays["held_lo"], outer.arrays["held_hi"])
    assert lib.zh_keyfan_schedule(None, pc.OUT_LEN, 4, C.byref(outer.tb), held) == inv
    assert lib.zh_keyfan_schedule(stage.handle, pc.OUT_LEN, 4, None, held) == inv
    assert lib.zh_keyfan_schedule(stage.handle, pc.OUT_LEN, 4, C.byref(outer.tb), None) == inv
    for broken in ((abi.ScriptSpanParam(), outer.arrays["held_hi"]), (outer.arrays["held_lo"], abi.ScriptSpanParam())):
        assert lib.zh_keyfan_schedule(stage.handle, pc.OUT_LEN, 4, C.byref(outer.tb), (abi.ScriptSpanParam * 2)(*broken)) == inv
    tb = outer.tb
    for broken in (abi.ScriptSpanTable(0, 0, tb.count, tb.start, tb.end, tb.note_id_changed), abi.ScriptSpanTable(4, 0, None, tb.start, tb.end, None),
                   abi.ScriptSpanTable(4, 0, tb.count, None, tb.end, None), abi.ScriptSpanTable(4, 0, tb.count, tb.start, None, None)):
        assert lib.zh_keyfan_schedule(stage.handle, pc.OUT_LEN, 4, C.byref(broken), held) == inv
    h = C.c_void_p()
    keys = np.zeros(65, np.float32)
    assert lib.zh_keyfan_create(ctx.handle, 1, keys.ctypes.data, 0, C.byref(h)) == inv
    assert lib.zh_keyfan_create(ctx.handle, 1, keys.ctypes.data, 65, C.byref(h)) == inv
    assert lib.zh_keyfan_create(ctx.handle, 1, None, 4, C.byref(h)) == inv
    assert lib.zh_keyfan_create(ctx.handle, 1, keys.ctypes.data, 4, None) == inv
    assert lib.zh_keyfan_create(None, 1, keys.ctypes.data, 4, C.byref(h)) == inv
    assert lib.zh_keyfan_create(ctx.handle, 2 ** 25 + 1, keys.ctypes.data, 64, C.byref(h)) == inv          # n_players * n_keys > 2^31
    assert lib.zh_keyfan_span_param(stage.handle, abi.KEYFAN_SPAN_FIELDS, C.byref(abi.ScriptSpanParam())) == inv
    assert lib.zh_keyfan_script_table(stage.handle, case.max_spans + 1, C.byref(abi.ScriptSpanTable())) == inv
    assert lib.zh_keyfan_reserve(stage.handle, 0) == inv
    assert lib.zh_keyfan_get_state(stage.handle, None) == inv and lib.zh_keyfan_set_state(stage.handle, None) == inv
    assert lib.zh_keyfan_overflows(stage.handle, None) == inv
    ctx.sync()
    assert stage.state().tobytes() == before and stage.overflows() == 0
    stage.close(); bank.close()
