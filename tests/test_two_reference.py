"""CPU: the model of the two-source tests (tests/two_reference.py) against tables written out by hand from
examples/example_two.zig:93-151 (tests/two_cases.py HAND): the sticky note_id_changed, a tie where both sources advance, a source
without rows, a source whose first row starts late, malformed ends -- and the model's MainModule against its own parts: the two
Triggers behind the loop give the rows the table form gives."""
import numpy as np
import pytest

from tests import two_cases as tc
from tests import two_reference as tr


@pytest.mark.parametrize("case", tc.HAND, ids=tc.HAND_IDS)
def test_merged_rows_equal_the_hand_written_table(case):
    got = tr.merge_player(case.a, tc.EXAMPLE.on_a, case.b, tc.EXAMPLE.on_b, tc.OUT_LEN)
    assert got == [(s, e, nic, list(w)) for s, e, nic, w in case.expect]


def test_the_sticky_nic_is_on_every_row_cut_from_one_source_row():
    rows = tr.merge_player([(0, 256, 1, (tc.F1, 1))], 1, [(0, 10, 0, (tc.C1, 0)), (10, 20, 0, (tc.C1, 0)), (20, 256, 0, (tc.C2, 0))], 1, 256)
    assert [r[3][5] for r in rows] == [1, 1, 1] and [r[2] for r in rows] == [1, 1, 1]


def test_the_table_form_drops_and_counts_rows_past_max_spans():
    pa, pb = tc.players(tc.PLAYERS)
    full, none = tr.merge_table(pa, 1, pb, 1, tc.OUT_LEN, tc.MAX_SPANS, 7)
    assert none == 0 and int(full["count"].max()) > 40
    cut, dropped = tr.merge_table(pa, 1, pb, 1, tc.OUT_LEN, 5, 7)
    assert dropped == int(np.maximum(full["count"].astype(np.int64) - 5, 0).sum()) > 0
    head = {k: (np.minimum(v, 5) if k == "count" else v[..., :5, :]) for k, v in full.items()}      # the first five rows of each list
    assert tr.same_table(head, cut) is None


def test_the_case_list_holds_what_the_mutants_need():
    """ties, sources that run out early, late first rows and rows beyond 34 + 34 - 1 cannot happen"""
    pa, pb = tc.players(tc.PLAYERS)
    ties = sum(len({r[1] for r in a} & {r[1] for r in b}) for a, b in zip(pa, pb))
    short = sum(a[-1][1] < tc.OUT_LEN or b[-1][1] < tc.OUT_LEN for a, b in zip(pa[len(tc.HAND):], pb[len(tc.HAND):]))
    late = sum(a[0][0] > 0 or b[0][0] > 0 for a, b in zip(pa, pb) if a and b)
    assert ties > 100 and short > 10 and late > 5
    assert max(len(tr.merge_player(a, 1, b, 1, tc.OUT_LEN)) for a, b in zip(pa, pb)) <= tc.MAX_SPANS


def test_main_modules_triggers_feed_the_same_loop(oracle):
    """MainModule's rows for scripted key events == the loop over the two Triggers' full sub-span lists as tables.  The lists come
    from a second body of trigger.zig, the library's host Trigger (zh_trigger_*), since the model's two faces share one."""
    from tests.lead_reference import Note                                      # (freq f32, note_on u32): the shape of both records
    from zang_amd import notes
    from zang_amd.zang import Span

    class ListTrigger:
        def __init__(self):
            self.t = notes.Trigger(Note)()

        def spans(self, start, end, impulses):
            iap = notes.ImpulsesAndParamses([notes.Impulse(f, i, 0) for f, i, _ in impulses], [Note(p[0], int(p[1])) for _, _, p in impulses])
            ctr = self.t.counter(Span(start, end), iap)
            return [(r.span.start, r.span.end, (r.params.freq, r.params.note_on), r.note_id_changed) for r in iter(lambda: self.t.next(ctr), None)]

    m = tr.MainModule(oracle)
    events = [(0, "k", 10, True, 30), (0, "n", 3, True, 30), (0, "k", 10, False, 90), (1, "k", 11, True, 0), (1, "n", 3, False, 17),
              (1, "n", 4, False, 40), (2, "k", 12, True, 255)]
    t0, t1 = ListTrigger(), ListTrigger()
    for b in range(3):
        for _, kind, key, down, frame in [e for e in events if e[0] == b]:
            m.key_event(key, down, frame, rel_freq=1.0 + key / 16 if kind == "k" else None, number=key if kind == "n" else None)
        m._first()
        i0, i1 = list(m.iq0.items), list(m.iq1.items)
        ctr0, ctr1 = m.trig0.counter(0, 256, m.iq0.consume()), m.trig1.counter(0, 256, m.iq1.consume())
        rows = tr.merge_loop(lambda: m.trig0.next(ctr0), lambda: m.trig1.next(ctr1), 0, 256)
        a = [(s, e, int(ch), (tc.fb(p[0]), int(p[1]))) for s, e, p, ch in t0.spans(0, 256, i0)]
        bb = [(s, e, int(ch), (tc.fb(p[0]), int(p[1]))) for s, e, p, ch in t1.spans(0, 256, i1)]
        want = tr.merge_player(a, 1, bb, 1, 256)
        got = [(s, e, int(tr.changed_of(n0, p0[1], n1, p1[1])), [tc.fb(p0[0]), int(p0[1]), tc.fb(p1[0]), int(p1[1]), int(tr.note_on_of(p0[1], p1[1])), int(n0), int(n1)])
               for s, e, p0, p1, n0, n1 in rows]
        assert got == want and rows[0][0] == 0 and rows[-1][1] == 256, b
    assert m.key0 == 12 and m.key1 is None and m.next_id0 == 6 and m.next_id1 == 4   # the release of number 4 was not the own key: no id drawn
