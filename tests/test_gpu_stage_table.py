"""GPU: the table contract the four span-table stages share (csrc/span_stage.hip.h) -- the arpeggiator, the subsong stage, the merge
stage and a live voice bank of polyphony 1 -- at 65 players (one full 64-lane block and one lane) and at none: the capacity's bounds,
reserve up, down and to the same capacity, the overflow count over two schedules, the spacing and kinds of the field arrays.  Inputs
are the existing cases' (tests/arp_cases.py, subsong_cases.py, two_cases.py), expected tables the Python models' (arp_reference.py,
subsong_reference.py, two_reference.py); the bank's expectation is the arpeggiator model's OUTER table.  Every table is brought to
two_reference's shape (count, start, end, nic, words [field][row][player]) and compared row by row below each player's count."""
import ctypes as C

import numpy as np
import pytest

from tests import arp_cases as ac
from tests import arp_reference as ar
from tests import subsong_cases as sc
from tests import subsong_reference as sr
from tests import test_gpu_arp as ga
from tests import test_gpu_span_merge as gm
from tests import test_gpu_subsong as gs
from tests import two_cases as tc
from tests import two_reference as tr

pytestmark = pytest.mark.gpu
N = 65
ARP_CASE = ac.CASES[1]                             # nd7: up to 37 ticks a call
SUBSONG_CASE = sc.case("more_than_32_events")


def _freq_on(tb):
    """an arp / subsong table (the model's or a downloaded one) with its words: freq as bits, note_on"""
    return dict(tb, words=np.stack([tb["freq"].view(np.uint32), tb["note_on"]]))


class Rig:
    """One stage with what feeds it.  `table`: the object whose table is under test (reserve, overflows, lib, handle); PREFIX: its
    C functions; ROWS: the capacity at creation; KINDS: per field "f", "u", or "b" (a bank's record word: either view).
    step(b, max_spans) schedules buffer b of the case; model(b, max_spans) -> (the expected table, the rows it drops)."""

    def schedule_rc(self, max_spans):
        """the return code of a schedule with nothing pushed"""
        raise NotImplementedError

    def views(self, max_spans):
        """-> (zh_*_script_table's return code, the table, the span param of every field)"""
        from zang_amd import abi
        lib, h = self.table.lib, self.table.handle
        tb, sp = abi.ScriptSpanTable(), [abi.ScriptSpanParam() for _ in self.KINDS]
        rc = getattr(lib, self.PREFIX + "_script_table")(h, max_spans, C.byref(tb))
        for f, p in enumerate(sp):
            assert getattr(lib, self.PREFIX + "_span_param")(h, f, C.byref(p)) == 0
        assert getattr(lib, self.PREFIX + "_span_param")(h, len(sp), C.byref(abi.ScriptSpanParam())) == abi.ZH_ERR_INVALID
        return rc, tb, sp


class ArpRig(Rig):
    """ARP_CASE through a bank and the arpeggiator"""
    PREFIX, ROWS, KINDS = "zh_arp", 4, "fu"

    def __init__(self, ctx, n):
        from zang_amd import arp
        self.arp, self.n, self.rec = arp, n, ac.run(ARP_CASE)
        self.bank, made, self.outer = ga._make(ctx, ARP_CASE, max(n, 1))     # no player: the stage reads nothing, any whole table passes
        made.close()
        self.table = self.stage = arp.ArpStage(ctx, n, ARP_CASE.key_freqs())

    def schedule_rc(self, max_spans):
        return self.stage._schedule(ARP_CASE.sample_rate, ac.OUT_LEN, max_spans, self.outer)

    def step(self, b, max_spans):
        ga._push(self.bank, self.rec.pushed[b][:self.n], self.arp.HELD_PARAMS)
        self.bank.schedule(ac.OUT_LEN, ac.OUTER_SPANS)
        assert self.schedule_rc(max_spans) == 0

    def model(self, b, max_spans):
        ref, dropped = ar.table(self.rec.inner[b][:self.n], max_spans)
        return _freq_on(ref), dropped

    def download(self, max_spans):
        return _freq_on(self.stage.download(max_spans))

    def close(self):
        self.stage.close(); self.bank.close()


class SubsongRig(Rig):
    """SUBSONG_CASE through a bank and the subsong stage"""
    PREFIX, ROWS, KINDS = "zh_subsong", 33, "fu"

    def __init__(self, ctx, n):
        from zang_amd import subsong
        self.subsong, self.n, self.rec = subsong, n, sc.run(SUBSONG_CASE)
        self.kit = subsong.MelodyKit(ctx, sc.KIT)
        self.bank, made, self.outer = gs._make(ctx, self.kit, SUBSONG_CASE, max(n, 1))
        made.close()
        self.table = self.stage = subsong.SubsongStage(ctx, n, self.kit, sc.BASE_FREQ)

    def schedule_rc(self, max_spans):
        return self.stage._schedule(sc.RATE, sc.OUT_LEN, max_spans, self.outer)

    def step(self, b, max_spans):
        gs._push(self.bank, SUBSONG_CASE, b, self.n, self.subsong.KEY_PARAMS)
        self.bank.schedule(sc.OUT_LEN, sc.OUTER_SPANS)
        assert self.stage._schedule(SUBSONG_CASE.rate(b), sc.OUT_LEN, max_spans, self.outer) == 0

    def model(self, b, max_spans):
        ref, dropped = sr.table(self.rec.inner[b][:self.n], max_spans)
        return _freq_on(ref), dropped

    def download(self, max_spans):
        return _freq_on(self.stage.download(max_spans))

    def close(self):
        self.stage.close(); self.bank.close(); self.kit.close()


class MergeRig(Rig):
    """two_cases' players through the merge stage; it keeps no state, so every buffer is the same one"""
    PREFIX, ROWS, KINDS = "zh_span_merge", 67, "fufuuuu"

    def __init__(self, ctx, n):
        self.pa, self.pb = tc.players(n) if n else ([], [])
        self.table = self.stage = gm._stage(ctx, n, tc.EXAMPLE)
        self.a, self.b = gm.DevSource(self.pa, "fu"), gm.DevSource(self.pb, "fu")

    def schedule_rc(self, max_spans):
        return gm._schedule(self.stage, self.a, self.b, tc.OUT_LEN, max_spans)

    def step(self, b, max_spans):
        assert self.schedule_rc(max_spans) == 0

    def model(self, b, max_spans):
        return gm._model(self.pa, self.pb, tc.EXAMPLE, max_spans)

    def download(self, max_spans):
        return gm._download(self.stage, max_spans)

    def close(self):
        self.stage.close()


class BankRig(Rig):
    """ARP_CASE's key events through a live bank of polyphony 1; the expectation is the arpeggiator model's outer table (its
    MainModule's Trigger), the record's words: held_lo, held_hi, on = 1"""
    PREFIX, ROWS, KINDS = "zh_voice_bank", 4, "bbb"

    def __init__(self, ctx, n):
        from zang_amd import arp
        from zang_amd.bank import LiveVoiceBank
        self.arp, self.n, self.rec = arp, n, ac.run(ARP_CASE)
        self.table = self.bank = LiveVoiceBank(ctx, n, 1, arp.HELD_PARAMS, arp.HELD_PARAMS.fields["on"][1], 33 * max(n, 1))

    def schedule_rc(self, max_spans):
        return self.bank.lib.zh_voice_bank_schedule_live(self.bank.handle, ac.OUT_LEN, max_spans, None)

    def step(self, b, max_spans):
        ga._push(self.bank, self.rec.pushed[b][:self.n], self.arp.HELD_PARAMS)
        self.bank.schedule(ac.OUT_LEN, max_spans)

    def model(self, b, max_spans):
        rows = [[(s, e, int(changed), [ac.mask_of(held) & 0xffffffff, ac.mask_of(held) >> 32, 1]) for s, e, held, changed in outer]
                for outer in self.rec.outer[b][:self.n]]
        return (tr.source_table([r[:max_spans] for r in rows], 3, max_spans), sum(max(0, len(r) - max_spans) for r in rows))

    def download(self, max_spans):
        got = self.bank.download(max_spans)
        return dict(got, nic=got["note_id_changed"])

    def close(self):
        self.bank.close()


rigs = pytest.mark.parametrize("Rig", [ArpRig, SubsongRig, MergeRig, BankRig], ids=["arp", "subsong", "merge", "bank"])


@rigs
def test_the_capacity_bounds_a_schedule_and_a_view(ctx, Rig):
    from zang_amd import abi
    r = Rig(ctx, N)
    for cap in (r.ROWS, r.ROWS + 13, 2):                               # as created, reserved up, reserved down
        r.table.reserve(cap)
        assert r.views(cap)[0] == 0 and r.views(cap + 1)[0] == abi.ZH_ERR_INVALID and r.views(0)[0] == abi.ZH_ERR_INVALID, cap
        assert r.schedule_rc(cap + 1) == abi.ZH_ERR_INVALID and r.schedule_rc(0) == abi.ZH_ERR_INVALID, cap
    assert getattr(r.table.lib, Rig.PREFIX + "_reserve")(r.table.handle, 0) == abi.ZH_ERR_INVALID
    r.close()


@rigs
def test_reserve_up_then_the_table_is_the_models(ctx, Rig):
    r = Rig(ctx, N)
    K = 80
    ref, dropped = r.model(0, K)
    assert int(ref["count"].max()) > 2
    r.table.reserve(K)
    r.step(0, K)
    got = r.download(K)
    assert tr.same_table(got, ref) is None, tr.same_table(got, ref)
    assert r.table.overflows() == dropped
    r.close()


@rigs
def test_reserve_down_stops_the_list_and_counts_what_is_dropped_over_two_schedules(ctx, Rig):
    r = Rig(ctx, N)
    K = 2
    refs = [r.model(b, K) for b in (0, 1)]
    assert all(d > 0 for _, d in refs), [d for _, d in refs]           # the model alone drops rows, in either buffer
    r.table.reserve(K)
    total = 0
    for b, (ref, dropped) in enumerate(refs):
        r.step(b, K)
        total += dropped
        assert r.table.overflows() == total, b
        got = r.download(K)
        assert int(got["count"].max()) == K and tr.same_table(got, ref) is None, (b, tr.same_table(got, ref))
    r.close()


@rigs
def test_reserve_to_the_same_capacity_keeps_the_table(ctx, Rig):
    r = Rig(ctx, N)
    K = 40
    r.table.reserve(K)
    r.step(0, K)
    ref, _ = r.model(0, K)
    before = r.download(K)
    r.table.reserve(K)
    after = r.download(K)
    assert tr.same_table(after, ref) is None, tr.same_table(after, ref)
    for name in ("count", "start", "end", "nic", "words"):             # every word of it, the rows above the counts too
        assert np.array_equal(np.asarray(before[name]), np.asarray(after[name])), name
    r.close()


@rigs
def test_the_field_arrays_are_a_plane_apart_and_of_their_kinds(ctx, Rig):
    r = Rig(ctx, N)
    for cap in (r.ROWS, 9):
        r.table.reserve(cap)
        ptrs = []
        for p, kind in zip(r.views(cap)[2], r.KINDS):
            assert (p.f is not None, p.u is not None) == (kind in "fb", kind in "ub"), (cap, kind)
            assert kind != "b" or p.f == p.u
            ptrs.append(p.f or p.u)
        assert [q - p for p, q in zip(ptrs, ptrs[1:])] == [cap * N * 4] * (len(ptrs) - 1), cap
    r.close()


@rigs
def test_no_players(ctx, Rig):
    r = Rig(ctx, 0)
    K = r.ROWS
    r.step(0, K)
    ctx.sync()
    assert r.table.overflows() == 0
    got = r.download(K)
    assert got["count"].shape == (0,) and all(got[name].shape == (K, 0) for name in ("start", "end", "nic"))
    assert len(got["words"]) == len(r.KINDS) and all(w.shape == (K, 0) for w in got["words"])
    r.close()
