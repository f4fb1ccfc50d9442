"""GPU: the arpeggiator stage (zh_arp_*, k_arp_schedule) behind a live voice bank of polyphony 1, against tests/arp_reference.py:
after each of six consecutive buffers of scripted key events the stage's table, counts, overflow counter and per-player state are
the model's, at every player count; a get_state / set_state round trip mid-sequence changes nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import arp_cases as ac
from tests import arp_reference as ar

pytestmark = pytest.mark.gpu


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
    from zang_amd import arp
    from zang_amd.bank import LiveVoiceBank
    bank = LiveVoiceBank(ctx, N, 1, arp.HELD_PARAMS, arp.HELD_PARAMS.fields["on"][1], 33 * N, rows=ac.OUTER_SPANS)
    stage = arp.ArpStage(ctx, N, case.key_freqs(), rows=case.max_spans)
    return bank, stage, arp.held_table(bank, ac.OUTER_SPANS)


@pytest.mark.parametrize("N", ac.PLAYERS)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.CASE_IDS)
def test_the_stage_equals_the_model_after_every_buffer(ctx, case, N):
    from zang_amd import abi, arp
    rec = ac.run(case)
    bank, stage, outer = _make(ctx, case, N)
    assert ac.state_words(stage.state()) == [[0, 1, -1, 0, 0, 0, 0]] * N                     # create == init()
    dropped = 0
    for b in range(ac.BUFFERS):
        _push(bank, rec.pushed[b][:N], arp.HELD_PARAMS)
        bank.schedule(ac.OUT_LEN, ac.OUTER_SPANS)
        stage.schedule(case.sample_rate, ac.OUT_LEN, case.max_spans, outer)
        ctx.sync()
        assert ctx.last_form() == ["k_arp_schedule"], ctx.last_form()
        got_outer = bank.download(ac.OUTER_SPANS)
        assert [int(c) for c in got_outer["count"]] == [len(o) for o in rec.outer[b][:N]], f"buffer {b}: the outer table"
        ref, d = ar.table(rec.inner[b][:N], case.max_spans)
        dropped += d
        got = stage.download(case.max_spans)
        assert ar.same_table(got, ref) is None, (f"buffer {b}", ar.same_table(got, ref))
        assert stage.overflows() == dropped, f"buffer {b}"
        assert ac.state_words(stage.state()) == rec.words[b][:N], f"buffer {b}: state"
        if b == 2:                                                   # a round trip mid-sequence changes nothing
            st = stage.state()
            stage.set_state(st)
            assert stage.state().tobytes() == st.tobytes()
    assert bank.overflows() == 0
    stage.close(); bank.close()


def test_a_set_state_is_where_the_model_goes_on_from(ctx):
    """the state after buffer 2 of one run set into a FRESH stage (and the outer bank's state into a fresh bank): buffers 3-5 are
    the model's"""
    from zang_amd import arp
    case, N = ac.CASES[2], 65
    rec = ac.run(case)
    bank, stage, outer = _make(ctx, case, N)
    for b in range(3):
        _push(bank, rec.pushed[b][:N], arp.HELD_PARAMS)
        bank.schedule(ac.OUT_LEN, ac.OUTER_SPANS)
    bank2, stage2, outer2 = _make(ctx, case, N)
    bank2.set_state(bank.get_state())
    stage2.set_state(ac.state_array(rec.words[2][:N], stage2.state().dtype))
    for b in range(3, ac.BUFFERS):
        _push(bank2, rec.pushed[b][:N], arp.HELD_PARAMS)
        bank2.schedule(ac.OUT_LEN, ac.OUTER_SPANS)
        stage2.schedule(case.sample_rate, ac.OUT_LEN, case.max_spans, outer2)
        ctx.sync()
        ref, _ = ar.table(rec.inner[b][:N], case.max_spans)
        got = stage2.download(case.max_spans)
        assert ar.same_table(got, ref) is None, (f"buffer {b}", ar.same_table(got, ref))
        assert ac.state_words(stage2.state()) == rec.words[b][:N], f"buffer {b}: state"
    for o in (stage, stage2, bank, bank2):
        o.close()


def test_reset_is_init(ctx):
    from zang_amd import arp
    case, N = ac.CASES[2], 3
    rec = ac.run(case)
    bank, stage, outer = _make(ctx, case, N)
    _push(bank, rec.pushed[0][:N], arp.HELD_PARAMS)
    bank.schedule(ac.OUT_LEN, ac.OUTER_SPANS)
    stage.schedule(case.sample_rate, ac.OUT_LEN, case.max_spans, outer)
    assert ac.state_words(stage.state()) == rec.words[0][:N] != [[0, 1, -1, 0, 0, 0, 0]] * N
    stage.reset()
    assert ac.state_words(stage.state()) == [[0, 1, -1, 0, 0, 0, 0]] * N
    stage.close(); bank.close()


def test_refusals(ctx):
    from zang_amd import abi, arp
    case, N = ac.CASES[2], 5
    bank, stage, outer = _make(ctx, case, N)
    before = stage.state().tobytes()
    for rate in ac.REJECTED_RATES:                                   # 1 <= note_duration < 2^31
        assert stage._schedule(rate, ac.OUT_LEN, case.max_spans, outer) == abi.ZH_ERR_INVALID, rate
    assert stage._schedule(case.sample_rate, ac.OUT_LEN, 0, outer) == abi.ZH_ERR_INVALID
    assert stage._schedule(case.sample_rate, ac.OUT_LEN, case.max_spans + 1, outer) == abi.ZH_ERR_INVALID      # above the capacity
    lib = ctx.lib
    held = (abi.ScriptSpanParam * 2)(outer.arrays["held_lo"], outer.arrays["held_hi"])
    assert lib.zh_arp_schedule(stage.handle, case.sample_rate, ac.OUT_LEN, 4, None, held) == abi.ZH_ERR_INVALID
    assert lib.zh_arp_schedule(stage.handle, case.sample_rate, ac.OUT_LEN, 4, C.byref(outer.tb), None) == abi.ZH_ERR_INVALID
    nohi = (abi.ScriptSpanParam * 2)(outer.arrays["held_lo"], abi.ScriptSpanParam())
    assert lib.zh_arp_schedule(stage.handle, case.sample_rate, ac.OUT_LEN, 4, C.byref(outer.tb), nohi) == abi.ZH_ERR_INVALID
    empty = abi.ScriptSpanTable(0, 0, outer.tb.count, outer.tb.start, outer.tb.end, outer.tb.note_id_changed)
    assert lib.zh_arp_schedule(stage.handle, case.sample_rate, ac.OUT_LEN, 4, C.byref(empty), held) == abi.ZH_ERR_INVALID
    h = C.c_void_p()
    keys = case.key_freqs()
    assert lib.zh_arp_create(ctx.handle, 1, keys.ctypes.data, 0, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_arp_create(ctx.handle, 1, keys.ctypes.data, 65, C.byref(h)) == abi.ZH_ERR_INVALID
    assert lib.zh_arp_create(ctx.handle, 1, None, 4, C.byref(h)) == abi.ZH_ERR_INVALID
    sp = abi.ScriptSpanParam()
    assert lib.zh_arp_span_param(stage.handle, abi.ARP_SPAN_FIELDS, C.byref(sp)) == abi.ZH_ERR_INVALID
    tb = abi.ScriptSpanTable()
    assert lib.zh_arp_script_table(stage.handle, case.max_spans + 1, C.byref(tb)) == abi.ZH_ERR_INVALID
    st = stage.state()
    for bad in (-2, case.n_keys):                                    # last_note indexes the key table
        st2 = st.copy()
        st2["last_note"][N - 1] = bad
        assert lib.zh_arp_set_state(stage.handle, st2.ctypes.data) == abi.ZH_ERR_INVALID
    ctx.sync()
    assert stage.state().tobytes() == before and stage.overflows() == 0
    stage.close(); bank.close()
