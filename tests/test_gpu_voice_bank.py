"""GPU: the voice bank (zh_voice_bank_*, csrc/sched_bank.hip) -- NoteTracker -> PolyphonyDispatcher -> Trigger for N instruments in
one kernel, filling the span tables on the device -- against the host scheduler (zh_poly_voice_schedule) and the reference's own
unit tests.  No tolerance anywhere: tables are integers and copied words, images are compared as bits."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import voice_bank_cases as vb

pytestmark = pytest.mark.gpu
SR = vb.SR
F = 1024


def _bank(ctx, P, offsets, rec, t, ids, rows=None):
    from zang_amd import bank
    return bank.VoiceBank(ctx, P, rec, offsets, t, ids, vb.ON_OFFSET, rows=rows)


# ------------------------------------------------------------------ 3. the reference's eight cases through the kernel
@pytest.mark.parametrize("case", vb.GOLDEN["trigger"], ids=lambda c: c["name"])
def test_trigger_reference_cases_through_the_kernel(ctx, case):
    rec, t, ids, expected = vb.trigger_case_song(case)
    b = _bank(ctx, 1, [0, len(t)], rec, t, ids, rows=8)
    for want in expected:
        b.schedule([1024], 1024.0, 8)
        d = b.download(8)
        got = [(int(d["start"][k, 0]), int(d["end"][k, 0]), int(d["words"][0][k, 0]), int(d["note_id_changed"][k, 0])) for k in range(int(d["count"][0]))]
        assert got == want
    assert b.overflows() == 0
    b.close()


@pytest.mark.parametrize("case", vb.GOLDEN["polyphony_dispatcher"], ids=lambda c: c["name"])
def test_dispatcher_reference_cases_through_the_kernel(ctx, case):
    rec, t, ids = vb.dispatcher_case_song(case)
    P = case["polyphony"]
    b = _bank(ctx, P, [0, len(t)], rec, t, ids, rows=8)
    b.schedule([1024], 1024.0, 8)
    d = b.download(8)
    got = [[int(d["words"][0][k, s].view(np.float32)) for k in range(int(d["count"][s]))] for s in range(P)]
    assert got == case["expected_note_ids"]
    b.close()


# ------------------------------------------------------------------ 4. equality with the host scheduler at scale
def _corpus_conditions(per_buffer, n_inst, P):
    """on the HOST result alone: the corpus exercises the code"""
    pairs = ge1 = ge3 = 0
    nic = [0, 0]
    for ref in per_buffer:
        pairs += len(ref["count"]); ge1 += int((ref["count"] >= 1).sum()); ge3 += int((ref["count"] >= 3).sum())
        m = vb.live(ref["count"], ref["start"].shape[0])
        ones = int(ref["note_id_changed"][m].sum())
        nic[1] += ones; nic[0] += int(m.sum()) - ones
    assert ge1 * 2 >= pairs and ge3 * 10 >= pairs, (ge1 / pairs, ge3 / pairs)
    assert nic[0] > 0 and nic[1] > 0


def _full_buffers(offsets, rec, t, ids, n_buffers):
    """(instrument, buffer) pairs where the host's NoteTracker delivers the full 32 impulses and more events than that fell into
    the buffer (they are dropped behind them); dense instruments only, the first four of them"""
    from zang_amd import abi
    L = abi.load()
    full = 0
    for i in [i for i in range(len(offsets) - 1) if i % 16 == 15][:4]:
        a, b = int(offsets[i]), int(offsets[i + 1])
        h = C.c_void_p()
        abi.check(L.zh_note_tracker_create(rec.dtype.itemsize, b - a, rec[a:b].ctypes.data, t[a:b].ctypes.data_as(C.POINTER(C.c_float)),
                                           ids[a:b].ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(h)), "create")
        clock, seen = np.float32(0.0), 0
        for _ in range(n_buffers):
            iap = abi.Iap()
            abi.check(L.zh_note_tracker_consume(h, SR, 0, F, C.byref(iap)), "consume")
            clock = np.float32(clock + np.float32(F) / np.float32(SR))
            upto = int(np.searchsorted(t[a:b], clock, side="left"))
            if iap.len == 32 and upto - seen > 32:
                full += 1
            seen = upto
        L.zh_note_tracker_destroy(h)
    return full


@pytest.mark.parametrize("n_inst,P", [(4096, 8), (1, 10), (1, 1), (64, 3)])
def test_bank_equals_the_host_scheduler(ctx, n_inst, P):
    B = 16
    offsets, rec, t, ids = vb.corpus(n_inst, B)
    host = vb.HostBank(P, offsets, rec, t, ids)
    per_buffer = [host.schedule([F]) for _ in range(B)]
    host.reset()
    whole = host.schedule([F] * B)
    host.close()
    if n_inst >= 64:
        _corpus_conditions(per_buffer, n_inst, P)
        assert _full_buffers(offsets, rec, t, ids, B) >= 1
    b = _bank(ctx, P, offsets, rec, t, ids, rows=34)
    for bi in range(B):                                            # one launch per buffer
        b.schedule([F], SR, 34)
        vb.assert_tables_equal(b.download(34), per_buffer[bi], f"buffer {bi}")
    K = int(whole["count"].max())
    b.reserve(K)
    b.reset()
    b.schedule([F] * B, SR, K)                                     # the same 16 as one launch
    vb.assert_tables_equal(b.download(K), whole, "n_buffers = 16")
    assert b.overflows() == 0
    b.close()


def test_more_buffers_than_one_launch_holds(ctx):
    """40 buffers in one call (the kernel takes 32 per launch), odd lengths among them"""
    P, n_inst = 3, 64
    frames = [F] * 40
    frames[7], frames[31], frames[32], frames[39] = 1, 777, 0, 417
    offsets, rec, t, ids = vb.corpus(n_inst, len(frames))
    host = vb.HostBank(P, offsets, rec, t, ids)
    whole = host.schedule(frames)
    host.close()
    K = int(whole["count"].max())
    b = _bank(ctx, P, offsets, rec, t, ids, rows=K)
    b.schedule(frames, SR, K)
    vb.assert_tables_equal(b.download(K), whole)
    b.close()


# ------------------------------------------------------------------ 5. overflow
def test_overflow_clamps_counts_and_later_buffers_are_unaffected(ctx):
    P, n_inst, B = 8, 256, 6
    offsets, rec, t, ids = vb.corpus(n_inst, B)
    host = vb.HostBank(P, offsets, rec, t, ids)
    refs = [host.schedule([F]) for _ in range(B)]
    host.close()
    b = _bank(ctx, P, offsets, rec, t, ids, rows=34)
    beyond = 0
    for bi in range(B - 1):
        b.schedule([F], SR, 2)
        ref = dict(refs[bi])
        beyond += int(np.maximum(ref["count"].astype(np.int64) - 2, 0).sum())
        ref["count"] = np.minimum(ref["count"], 2)
        vb.assert_tables_equal(b.download(2), ref, f"buffer {bi}")
    assert beyond > 0 and b.overflows() == beyond
    b.schedule([F], SR, 34)
    vb.assert_tables_equal(b.download(34), refs[B - 1], "the buffer after the overflows")
    assert b.overflows() == beyond
    b.close()


# ------------------------------------------------------------------ 6. state
def test_reset_and_state_round_trip(ctx):
    P, n_inst = 3, 64
    offsets, rec, t, ids = vb.corpus(n_inst, 10)
    b = _bank(ctx, P, offsets, rec, t, ids, rows=34)

    def run(n):
        out = []
        for _ in range(n):
            b.schedule([F], SR, 34)
            out.append(b.download(34))
        return out
    first = run(5)
    state = b.get_state()
    assert any(s.next_event > 0 for s in state[0]) and any(v.has_note for v in state[1]) and any(v.used for v in state[1])
    second = run(5)
    b.set_state(state)
    again = run(5)
    for x, y in zip(second, again):
        vb.assert_tables_equal(y, x, "after set_state")
    b.reset()
    for x, y in zip(first, run(5)):
        vb.assert_tables_equal(y, x, "after reset")
    b.close()


# ------------------------------------------------------------------ 7. end to end, bits
def _host_span_table(ref, device):
    from zang_amd.spans import SpanTable
    K = max(int(ref["count"].max()), 1)
    return SpanTable.from_arrays(ref["count"], ref["start"][:K], ref["end"][:K], ref["words"][0][:K].view(np.float32), ref["note_on"][:K],
                                 ref["note_id_changed"][:K], device)


def test_nice_and_pulseosc_over_bank_tables_equal_host_made_tables(ctx):
    from zang_amd import modules as mod, zang
    P, n_inst, B = 8, 64, 6
    V = n_inst * P
    offsets, rec, t, ids = vb.corpus(n_inst, B)
    host = vb.HostBank(P, offsets, rec, t, ids)
    b = _bank(ctx, P, offsets, rec, t, ids, rows=34)
    nice_h, nice_d = mod.NiceInstrument(V, 0.25, ctx), mod.NiceInstrument(V, 0.25, ctx)
    osc_h, osc_d = mod.PulseOsc(V, ctx), mod.PulseOsc(V, ctx)
    imgs = [ctx.image(F, V) for _ in range(4)]
    span = zang.Span(0, F)
    params = mod.PulseOsc.Params(SR, zang.constant(440.0), 0.5)
    for bi in range(B):
        ref = host.schedule([F])
        K = max(int(ref["count"].max()), 1)
        nice_h.paint_spans(span, [imgs[0]], None, SR, _host_span_table(ref, ctx.device), zero_first=True)
        osc_h.paint_spans(span, [imgs[2]], [], params, mod.PulseOsc.span_table(ref["count"], ref["start"][:K], ref["end"][:K], ref["note_id_changed"][:K],
                                                                               {"freq": (ref["words"][0][:K].view(np.float32), None)}), zero_first=True)
        b.schedule([F], SR, 34)
        nice_d.paint_spans(span, [imgs[1]], None, SR, b.span_table(34, 0), zero_first=True)
        osc_d.paint_spans(span, [imgs[3]], [], params, b.script_table(34, {"freq": (0, "f")}), zero_first=True)
        ctx.sync()
        got = [i.cpu().numpy().view(np.uint32) for i in imgs]
        assert np.array_equal(got[0], got[1]), ("nice", bi)
        assert np.array_equal(got[2], got[3]), ("pulseosc", bi)
        assert got[0].any() and got[2].any()
    host.close()
    b.close()


def test_song_renderer_device_scheduler_equals_host_and_oracle_60s(ctx, oracle):
    from tests.test_song import REF_SONG, _oracle_song_render
    from zang_amd import song
    text = open(REF_SONG).read()
    seconds = 60.0
    rh = song.SongRenderer(text, ctx)
    want = rh.render(seconds)
    rd = song.SongRenderer(text, ctx, scheduler="device")
    got = rd.render(seconds)
    assert len(got) == int(seconds * SR) * 2 and got == want
    total = int(seconds * SR)
    nbuf = (total + F - 1) // F
    ref = _oracle_song_render(oracle, rh.notes, song.EXAMPLE_SONG_INSTRUMENTS, nbuf, last_frames=total - (nbuf - 1) * F)
    assert got == ref
    # and buffer by buffer (render_buffer)
    r1, r2 = song.SongRenderer(text, ctx), song.SongRenderer(text, ctx, scheduler="device")
    for _ in range(40):
        assert r1.render_buffer() == r2.render_buffer()
    assert all(b.overflows() == 0 for b in rd.banks + r2.banks)


def test_poly_script_voice_device_route_equals_host_route(ctx):
    import torch
    from tests.test_gpu_script_spans import EXAMPLE, _demo_events, _program
    from zang_amd import script, zang
    sr, B, P = 44100.0, 8, 8
    prog = _program(ctx, EXAMPLE, "DemoPlayer")
    try:
        events = _demo_events(np.random.default_rng(8), 40, B * F / sr)
        mh, md = prog.module("DemoPlayer", P), prog.module("DemoPlayer", P)
        ph = script.PolyScriptVoice(mh, P, ["freq", "note_on"], events)
        pd = script.PolyScriptVoice(md, P, ["freq", "note_on"], events, device=True)
        ih, idv = ctx.image(F, P), ctx.image(F, P)
        sound = False
        for b in range(B):
            ph.paint(zang.Span(0, F), [ih], {"sample_rate": sr}, sr)
            pd.paint(zang.Span(0, F), [idv], {"sample_rate": sr}, sr)
            ctx.sync()
            a, c = ih.cpu().numpy().view(np.uint32), idv.cpu().numpy().view(np.uint32)
            assert np.array_equal(a, c), b
            sound = sound or bool(a.any())
        assert sound
        ph.close(); pd.close()
    finally:
        prog.close()


# ------------------------------------------------------------------ 8. capture
def _side_context():
    """a context on a stream of its own (the legacy default stream cannot be captured)"""
    import torch
    import zang_amd
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        return zang_amd.Context(0), side


def test_captured_schedule_and_paint_replays_twelve_buffers(ctx):
    from zang_amd import modules as mod, zang
    P, n_inst, B = 8, 64, 12
    V = n_inst * P
    offsets, rec, t, ids = vb.corpus(n_inst, B)
    host = vb.HostBank(P, offsets, rec, t, ids)
    c2, _side = _side_context()
    b = _bank(c2, P, offsets, rec, t, ids, rows=34)
    nice_h, nice_d = mod.NiceInstrument(V, 0.25, ctx), mod.NiceInstrument(V, 0.25, c2)
    img_h, img_d = ctx.image(F, V), c2.image(F, V)
    span = zang.Span(0, F)
    table = b.span_table(34, 0)
    c2.sync()

    def body():
        b.schedule([F], SR, 34)
        nice_d.paint_spans(span, [img_d], None, SR, table, zero_first=True)
    g = c2.capture(body)                                           # recorded ONCE
    assert "k_voice_bank_schedule" in [k for k, _ in g.kernels()]
    for bi in range(B):
        nice_h.paint_spans(span, [img_h], None, SR, _host_span_table(host.schedule([F]), ctx.device), zero_first=True)
        g.launch()
        ctx.sync(); c2.sync()
        assert np.array_equal(img_h.cpu().numpy().view(np.uint32), img_d.cpu().numpy().view(np.uint32)), bi
    assert b.overflows() == 0
    g.close()
    host.close()
    b.close()
    c2.close()


def test_schedule_names_its_kernel_and_reserve_is_refused_in_a_capture(ctx):
    from zang_amd import abi
    offsets, rec, t, ids = vb.corpus(4, 2)
    c2, _side = _side_context()
    b = _bank(c2, 3, offsets, rec, t, ids)
    b.schedule([F], SR, 4)
    assert c2.last_form() == ["k_voice_bank_schedule"]
    c2.sync()
    rcs = []

    def body():
        rcs.append(c2.lib.zh_voice_bank_reserve(b.handle, 9))
        b.schedule([F], SR, 4)
    g = c2.capture(body)
    g.close()
    assert rcs == [abi.ZH_ERR_UNSUPPORTED]
    b.close()
    c2.close()


# ------------------------------------------------------------------ 9. refusals and the empty bank
def test_refusals_and_the_empty_bank(ctx):
    from zang_amd import abi
    L = ctx.lib
    offsets, rec, t, ids = vb.corpus(2, 2)
    h = C.c_void_p()

    def create(n=2, P=3, size=8, on=4, off=offsets, r=rec, tt=t, ii=ids, ctxh=ctx.handle, out=C.byref(h)):
        return L.zh_voice_bank_create(ctxh, n, P, size, on, off.ctypes.data if off is not None else None, r.ctypes.data if r is not None else None,
                                      tt.ctypes.data if tt is not None else None, ii.ctypes.data if ii is not None else None, out)
    bad = abi.ZH_ERR_INVALID
    assert create(ctxh=None) == bad and create(out=None) == bad and create(P=0) == bad
    assert create(size=0) == bad and create(size=6) == bad and create(size=68) == bad and create(on=8) == bad
    assert create(off=None) == bad and create(r=None) == bad and create(tt=None) == bad and create(ii=None) == bad
    assert create(off=np.array([0, 9, 5], np.uint64)) == bad and create(off=np.array([1, 5, 9], np.uint64)) == bad
    assert create() == abi.ZH_OK and h
    fr = np.array([F], np.uint32)
    assert L.zh_voice_bank_schedule(None, SR, fr.ctypes.data, 1, 4) == bad
    assert L.zh_voice_bank_schedule(h, SR, None, 1, 4) == bad
    assert L.zh_voice_bank_schedule(h, SR, fr.ctypes.data, 1, 0) == bad
    assert L.zh_voice_bank_schedule(h, SR, fr.ctypes.data, 1, 5) == bad                  # above the capacity (4 rows at creation)
    assert L.zh_voice_bank_reserve(h, 0) == bad and L.zh_voice_bank_reserve(None, 4) == bad
    assert L.zh_voice_bank_reserve(h, 5) == abi.ZH_OK and L.zh_voice_bank_schedule(h, SR, fr.ctypes.data, 1, 5) == abi.ZH_OK
    tb, sp, st = abi.ScriptSpanTable(), abi.ScriptSpanParam(), abi.SpanTable()
    assert L.zh_voice_bank_script_table(h, 6, C.byref(tb)) == bad and L.zh_voice_bank_script_table(h, 0, C.byref(tb)) == bad
    assert L.zh_voice_bank_script_table(h, 5, None) == bad and L.zh_voice_bank_script_table(None, 5, C.byref(tb)) == bad
    assert L.zh_voice_bank_span_param(h, 2, C.byref(sp)) == bad and L.zh_voice_bank_span_param(h, 1, C.byref(sp)) == abi.ZH_OK and sp.f == sp.u
    assert L.zh_voice_bank_span_table(h, 5, 2, C.byref(st)) == bad and L.zh_voice_bank_span_table(h, 5, 0, C.byref(st)) == abi.ZH_OK
    assert L.zh_voice_bank_overflows(h, None) == bad and L.zh_voice_bank_get_state(h, None, None) == bad
    assert L.zh_voice_bank_reset(None) == bad and L.zh_voice_bank_destroy(None) == bad
    assert L.zh_voice_bank_destroy(h) == abi.ZH_OK
    # zero instruments: ZH_OK, nothing runs
    e = C.c_void_p()
    assert L.zh_voice_bank_create(ctx.handle, 0, 3, 8, 4, None, None, None, None, C.byref(e)) == abi.ZH_OK
    assert L.zh_voice_bank_schedule(e, SR, fr.ctypes.data, 1, 4) == abi.ZH_OK
    n = C.c_uint64(7)
    assert L.zh_voice_bank_overflows(e, C.byref(n)) == abi.ZH_OK and n.value == 0
    assert L.zh_voice_bank_get_state(e, None, None) == abi.ZH_OK and L.zh_voice_bank_reset(e) == abi.ZH_OK
    assert L.zh_voice_bank_destroy(e) == abi.ZH_OK
