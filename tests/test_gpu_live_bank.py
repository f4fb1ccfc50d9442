"""GPU: live voice banks (zh_voice_bank_create_live / _schedule_live, k_voice_bank_schedule_live in csrc/sched_bank.hip) -- ImpulseQueue ->
PolyphonyDispatcher -> Trigger for N instruments in one kernel from impulses pushed per buffer -- against the host classes composed per
instrument (tests/live_bank_cases.py), against a song bank fed the same events, and through the paints.  No tolerance anywhere: tables
are integers and copied words, images and module states are compared as bits."""
import ctypes as C

import numpy as np
import pytest

from tests import live_bank_cases as lb
from tests import voice_bank_cases as vb

pytestmark = pytest.mark.gpu
SR = vb.SR


def _live(ctx, n_inst, P, max_impulses, rows=lb.ROWS, dtype=lb.REC, on_offset=lb.ON_OFFSET):
    from zang_amd import bank
    return bank.LiveVoiceBank(ctx, n_inst, P, dtype, on_offset, max_impulses, rows=rows)


def _most(buffers):
    return max(len(b[1]) for b in buffers)


# ------------------------------------------------------------------ 1. tables and state equal the host composition
@pytest.mark.parametrize("n_inst,P", [(n, P) for n in (1, 63, 65, 130) for P in (1, 3, 8)] + [(5, 200)])
def test_live_bank_equals_the_host_composition(ctx, n_inst, P):
    """24 buffers (1,024 frames; single ones of 1, 0, 777 and 1,023).  1 / 63 / 65 / 130 instruments: one workgroup not full, full less one,
    one more than full, three with a ragged last; polyphony 200: 32 instruments per workgroup instead of 64."""
    buffers = lb.corpus(n_inst)
    refs, host = lb.reference(n_inst, P)
    if n_inst >= 63:
        lb.assert_coverage(host.stats, len(buffers))
    b = _live(ctx, n_inst, P, _most(buffers))
    for bi, (out_len, inst, frame, ids, rec) in enumerate(buffers):
        b.push(inst, frame, ids, rec)
        b.schedule(out_len, lb.ROWS)
        vb.assert_tables_equal(b.download(lb.ROWS), refs[bi], f"buffer {bi}")
    assert b.overflows() == 0
    next_id, voices = b.get_state()
    lb.assert_state_equal(next_id, voices, host, "after the last buffer")
    b.close()


def test_overflow_clamps_counts_and_later_buffers_are_unaffected(ctx):
    n_inst, P = 65, 3
    buffers = lb.corpus(n_inst)
    refs, _ = lb.reference(n_inst, P)
    b = _live(ctx, n_inst, P, _most(buffers))
    beyond = 0
    for bi in range(6):
        b.push(*buffers[bi][1:])
        b.schedule(buffers[bi][0], 2)
        ref = dict(refs[bi])
        beyond += int(np.maximum(ref["count"].astype(np.int64) - 2, 0).sum())
        ref["count"] = np.minimum(ref["count"], 2)
        vb.assert_tables_equal(b.download(2), ref, f"buffer {bi}")
    assert beyond > 0 and b.overflows() == beyond
    b.push(*buffers[6][1:])
    b.schedule(buffers[6][0], lb.ROWS)
    vb.assert_tables_equal(b.download(lb.ROWS), refs[6], "the buffer after the overflows")
    assert b.overflows() == beyond
    b.close()


# ------------------------------------------------------------------ 2. a live bank fed a song's impulses equals the song bank
def test_live_bank_fed_the_trackers_impulses_equals_the_song_bank(ctx):
    """15 instruments of the song corpus (none of the dense ones), polyphony 4: per buffer the impulses zh_note_tracker_consume delivers,
    pushed; every array of the live bank's tables equals the song bank's (zh_voice_bank_schedule, one buffer per call)."""
    from zang_amd import abi, bank
    L = abi.load()
    n_inst, P = 15, 4
    frames = [1024] * 12
    frames[4], frames[9] = 777, 1
    offsets, rec, t, ids = vb.corpus(n_inst, len(frames))
    song = bank.VoiceBank(ctx, P, rec, offsets, t, ids, vb.ON_OFFSET, rows=lb.ROWS)
    live = _live(ctx, n_inst, P, 32 * n_inst, dtype=vb.REC, on_offset=vb.ON_OFFSET)
    trackers = []
    for i in range(n_inst):
        a, z = int(offsets[i]), int(offsets[i + 1])
        h = C.c_void_p()
        abi.check(L.zh_note_tracker_create(rec.dtype.itemsize, z - a, rec[a:z].ctypes.data, t[a:z].ctypes.data_as(C.POINTER(C.c_float)),
                                           ids[a:z].ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(h)), "zh_note_tracker_create")
        trackers.append(h)
    spans = 0
    for bi, n in enumerate(frames):
        for i, h in enumerate(trackers):
            iap = abi.Iap()
            abi.check(L.zh_note_tracker_consume(h, SR, 0, n, C.byref(iap)), "zh_note_tracker_consume")
            assert iap.len < 32, "an instrument-buffer that may hold more than 32 events: the tracker would have dropped some"
            k = int(iap.len)
            if k:
                recs = np.frombuffer(C.string_at(iap.paramses, k * rec.dtype.itemsize), rec.dtype)
                live.push(np.full(k, i, np.uint32), [iap.impulses[j].frame for j in range(k)], [iap.impulses[j].note_id for j in range(k)], recs)
        song.schedule([n], SR, lb.ROWS)
        live.schedule(n, lb.ROWS)
        want, got = song.download(lb.ROWS), live.download(lb.ROWS)
        vb.assert_tables_equal(got, want, f"buffer {bi}")
        spans += int(want["count"].sum())
    assert spans > n_inst * P * len(frames) // 2 and song.overflows() == 0 and live.overflows() == 0
    for h in trackers:
        L.zh_note_tracker_destroy(h)
    song.close(); live.close()


# ------------------------------------------------------------------ 3. the views feed the paints
def test_nice_and_pulseosc_over_live_bank_views_equal_host_made_tables(ctx):
    from zang_amd import modules as mod, zang
    from zang_amd.spans import SpanTable
    n_inst, P, F = 5, 3, 256
    V = n_inst * P
    frames = (F,) * 6
    buffers = lb.corpus(n_inst, lb.SEED + 1, frames)
    refs, _ = lb.reference(n_inst, P, lb.SEED + 1, frames)
    b = _live(ctx, n_inst, P, _most(buffers))
    nice_h, nice_d = mod.NiceInstrument(V, 0.25, ctx), mod.NiceInstrument(V, 0.25, ctx)
    osc_h, osc_d = mod.PulseOsc(V, ctx), mod.PulseOsc(V, ctx)
    imgs = [ctx.image(F, V) for _ in range(4)]
    span = zang.Span(0, F)
    params = mod.PulseOsc.Params(SR, zang.constant(440.0), 0.5)
    table, script = b.span_table(lb.ROWS, 0), b.script_table(lb.ROWS, {"freq": (0, "f")})       # made once: the addresses stay
    for bi, (out_len, inst, frame, ids, rec) in enumerate(buffers):
        ref = refs[bi]
        K = max(int(ref["count"].max()), 1)
        freq = ref["words"][0][:K].view(np.float32)
        nice_h.paint_spans(span, [imgs[0]], None, SR, SpanTable.from_arrays(ref["count"], ref["start"][:K], ref["end"][:K], freq, ref["note_on"][:K],
                                                                            ref["note_id_changed"][:K], ctx.device), zero_first=True)
        osc_h.paint_spans(span, [imgs[2]], [], params, mod.PulseOsc.span_table(ref["count"], ref["start"][:K], ref["end"][:K], ref["note_id_changed"][:K],
                                                                               {"freq": (freq, None)}), zero_first=True)
        b.push(inst, frame, ids, rec)
        b.schedule(out_len, lb.ROWS)
        nice_d.paint_spans(span, [imgs[1]], None, SR, table, zero_first=True)
        osc_d.paint_spans(span, [imgs[3]], [], params, script, zero_first=True)
        ctx.sync()
        got = [i.cpu().numpy().view(np.uint32) for i in imgs]
        assert np.array_equal(got[0], got[1]), ("nice", bi)
        assert np.array_equal(got[2], got[3]), ("pulseosc", bi)
        assert nice_h.state().tobytes() == nice_d.state().tobytes(), ("nice state", bi)
        assert osc_h.state().tobytes() == osc_d.state().tobytes(), ("pulseosc state", bi)
    assert got[0].any() and got[2].any()
    b.close()


# ------------------------------------------------------------------ 4. state
def test_state_round_trip_in_the_middle_of_a_stream_and_reset(ctx):
    n_inst, P = 65, 3
    buffers = lb.corpus(n_inst)
    refs, _ = lb.reference(n_inst, P)
    a = _live(ctx, n_inst, P, _most(buffers))

    def run(bank, lo, hi):
        out = []
        for out_len, inst, frame, ids, rec in buffers[lo:hi]:
            bank.push(inst, frame, ids, rec)
            bank.schedule(out_len, lb.ROWS)
            out.append(bank.download(lb.ROWS))
        return out
    run(a, 0, 9)
    state = a.get_state()
    assert all(x > 1 for x in state[0][:n_inst]) and any(v.has_note for v in state[1]) and any(v.used for v in state[1])
    fresh = _live(ctx, n_inst, P, _most(buffers))                     # another bank takes the stream over
    fresh.set_state(state)
    for bi, (x, y) in enumerate(zip(run(a, 9, 16), run(fresh, 9, 16))):
        vb.assert_tables_equal(y, x, "restored bank")
        vb.assert_tables_equal(x, refs[9 + bi], "original bank")
    a.set_state(state)                                               # and the same bank goes back
    for bi, y in enumerate(run(a, 9, 12)):
        vb.assert_tables_equal(y, refs[9 + bi], "after set_state")
    # reset: dispatcher and Triggers cleared, next_event_id kept
    before = a.get_state()[0].copy()
    a.reset()
    after = a.get_state()
    assert np.array_equal(after[0], before) and not any(v.used or v.has_note for v in after[1])
    a.schedule(64, lb.ROWS)
    assert not a.download(lb.ROWS)["count"].any()
    a.close(); fresh.close()


# ------------------------------------------------------------------ 5. misuse
def _one_push(inst=0):
    return (np.array([inst], np.uint32), np.array([3], np.uint32), np.array([1], np.uint64), np.array([(440.0, 1, (0, 0, 0), 7)], lb.REC))


def _batch(arrays, n=None):
    from zang_amd import abi
    inst, frame, ids, rec = arrays
    c = abi.BankImpulses(len(inst) if n is None else n, inst.ctypes.data, frame.ctypes.data, ids.ctypes.data, rec.ctypes.data)
    c._keep = arrays
    return c


def test_song_schedule_on_a_live_bank_is_refused(ctx):
    from zang_amd import abi
    b = _live(ctx, 2, 3, 8)
    fr = np.array([64], np.uint32)
    assert ctx.lib.zh_voice_bank_schedule(b.handle, SR, fr.ctypes.data, 1, 4) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_voice_bank_get_state(b.handle, None, None) == abi.ZH_ERR_INVALID
    b.close()


def test_live_schedule_on_a_song_bank_is_refused(ctx):
    from zang_amd import abi, bank
    offsets, rec, t, ids = vb.corpus(2, 2)
    s = bank.VoiceBank(ctx, 3, rec, offsets, t, ids, vb.ON_OFFSET)
    assert ctx.lib.zh_voice_bank_schedule_live(s.handle, 64, 4, None) == abi.ZH_ERR_INVALID
    nid = (C.c_uint64 * 2)()
    assert ctx.lib.zh_voice_bank_live_get_state(s.handle, nid, (abi.VoiceBankLiveVoiceState * 6)()) == abi.ZH_ERR_INVALID
    s.close()


def test_an_instrument_index_out_of_range_is_refused(ctx):
    from zang_amd import abi
    b = _live(ctx, 2, 3, 8)
    assert ctx.lib.zh_voice_bank_schedule_live(b.handle, 64, 4, C.byref(_batch(_one_push(2)))) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_voice_bank_schedule_live(b.handle, 64, 4, C.byref(_batch(_one_push(1)))) == abi.ZH_OK
    assert b.download(4)["count"].tolist() == [0, 0, 0, 1, 0, 0]
    b.close()


def test_a_batch_above_max_impulses_is_refused(ctx):
    from zang_amd import abi
    b = _live(ctx, 2, 3, 2, rows=None)
    three = tuple(np.concatenate([x] * 3) for x in _one_push())
    assert ctx.lib.zh_voice_bank_schedule_live(b.handle, 64, 4, C.byref(_batch(three))) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_voice_bank_schedule_live(b.handle, 64, 4, C.byref(_batch(three, 2))) == abi.ZH_OK
    assert ctx.lib.zh_voice_bank_schedule_live(b.handle, 64, 0, None) == abi.ZH_ERR_INVALID
    assert ctx.lib.zh_voice_bank_schedule_live(b.handle, 64, 5, None) == abi.ZH_ERR_INVALID       # above the capacity (4 rows at creation)
    assert ctx.lib.zh_voice_bank_schedule_live(None, 64, 4, None) == abi.ZH_ERR_INVALID
    b.close()


def test_the_live_call_is_unsupported_while_a_capture_records(ctx):
    import torch
    import zang_amd
    from zang_amd import abi, zang
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = zang_amd.Context(0)
    b = _live(c2, 2, 3, 8)
    b.schedule(64, 4)
    assert c2.last_form() == ["k_voice_bank_schedule_live"]
    c2.sync()
    rcs = []

    def body():
        rcs.append(c2.lib.zh_voice_bank_schedule_live(b.handle, 64, 4, None))
        rcs.append(c2.lib.zh_voice_bank_schedule_live(b.handle, 64, 4, C.byref(_batch(_one_push()))))
        zang.zero(zang.Span(0, 8), img, c2)                            # (an empty capture is not the point)
    img = c2.image(8, 2)
    g = c2.capture(body)
    g.close()
    assert rcs == [abi.ZH_ERR_UNSUPPORTED] * 2
    b.close()
    c2.close()


def test_reserve_invalidates_views_as_documented(ctx):
    """a reserve that changes the capacity frees the tables: a view made before it is stale, one made after it sees the next buffer"""
    b = _live(ctx, 2, 3, 8, rows=4)
    old = b.span_table(4, 0)
    b.reserve(9)
    new = b.span_table(9, 0)
    assert new.c.max_spans == 9 and old.c.max_spans == 4
    b.push(*_one_push(1))
    b.schedule(64, 9)
    d = b.download(9)
    assert d["count"].tolist() == [0, 0, 0, 1, 0, 0] and (int(d["start"][0, 3]), int(d["end"][0, 3])) == (3, 64)
    b.reserve(9)                                                     # the same capacity: nothing moves
    same = b.span_table(9, 0)
    assert (same.c.count, same.c.start, same.c.freq) == (new.c.count, new.c.start, new.c.freq)
    from zang_amd import abi
    assert ctx.lib.zh_voice_bank_reserve(b.handle, 0) == abi.ZH_ERR_INVALID
    b.close()


def test_zero_instruments_and_an_empty_batch_are_ok(ctx):
    from zang_amd import abi
    L = ctx.lib
    e = C.c_void_p()
    assert L.zh_voice_bank_create_live(ctx.handle, 0, 3, 12, 4, 8, C.byref(e)) == abi.ZH_OK
    assert L.zh_voice_bank_schedule_live(e, 64, 4, None) == abi.ZH_OK
    n = C.c_uint64(7)
    assert L.zh_voice_bank_overflows(e, C.byref(n)) == abi.ZH_OK and n.value == 0
    assert L.zh_voice_bank_live_get_state(e, None, None) == abi.ZH_OK and L.zh_voice_bank_reset(e) == abi.ZH_OK
    assert L.zh_voice_bank_destroy(e) == abi.ZH_OK
    b = _live(ctx, 3, 2, 0)                                          # a bank that never takes a push
    b.schedule(64, 4)
    empty = _batch(_one_push(), 0)
    assert L.zh_voice_bank_schedule_live(b.handle, 64, 4, C.byref(empty)) == abi.ZH_OK
    assert not b.download(4)["count"].any() and b.overflows() == 0
    bad = abi.ZH_ERR_INVALID
    h = C.c_void_p()
    assert L.zh_voice_bank_create_live(ctx.handle, 2, 0, 12, 4, 8, C.byref(h)) == bad and L.zh_voice_bank_create_live(ctx.handle, 2, 3, 10, 4, 8, C.byref(h)) == bad
    assert L.zh_voice_bank_create_live(ctx.handle, 2, 3, 12, 12, 8, C.byref(h)) == bad and L.zh_voice_bank_create_live(None, 2, 3, 12, 4, 8, C.byref(h)) == bad
    b.close()
