"""Shared by tests/test_live_bank_host.py (CPU) and tests/test_gpu_live_bank.py: the seeded corpus of pushed impulses and the
reference for a live voice bank -- the host classes composed per instrument and per buffer, exactly as the header states it:
zh_impulse_queue_push in batch order, zh_impulse_queue_consume, zh_polyphony_dispatcher_dispatch, zh_trigger_counter(0, out_len) and
zh_trigger_next per slot -- assembled into bank-shaped tables.  The host classes are opaque, so the state the device is compared with
(slots, Trigger notes, carried records, next_event_id) is derived from what they return; every record carries a unique tag word for that."""
import ctypes as C
import functools

import numpy as np

from tests import voice_bank_cases as vb
from zang_amd import abi

ROOT = vb.ROOT
GOLDEN = vb.GOLDEN
REC = np.dtype([("freq", "<f4"), ("on", "u1"), ("pad", "u1", 3), ("tag", "<u4")])     # MyNoteParams {freq, note_on} + a serial number
W = REC.itemsize // 4
ON_OFFSET = 4
TAG_WORD = 2
SEED = 20261018
ROWS = 34                                    # 32 impulses per buffer: at most 33 sub-spans per voice
FRAMES = tuple(1024 if i not in (3, 7, 12, 18) else {3: 1, 7: 0, 12: 777, 18: 1023}[i] for i in range(24))


@functools.lru_cache(maxsize=None)
def corpus(n_instruments, seed=SEED, frames=FRAMES):
    """one buffer per entry of `frames` (24 by default); per instrument and buffer a Poisson(3) number of pushes (one instrument in 16: 40), frames ascending except that 5 %
    lie below their predecessor's, some equal it, some sit at out_len - 1 and a few at or above out_len; note ids 1..6, note_on with
    probability 0.6.  The instruments' pushes are interleaved at random (each instrument's own order kept).
    -> per buffer (out_len, instrument u32[], frame u32[], note_id u64[], records REC[])"""
    rng = np.random.default_rng(seed)
    tag, out = 1, []
    for L in frames:
        per = []
        for i in range(n_instruments):
            k = 40 if i % 16 == 15 else int(rng.poisson(3))
            fr = np.sort(rng.integers(0, max(L, 1), k)).astype(np.int64)
            for j in range(1, k):
                u = rng.random()
                if u < 0.05 and fr[j - 1] > 0:
                    fr[j] = rng.integers(0, fr[j - 1])               # below its predecessor's: dropped if that one was accepted
                elif u < 0.20:
                    fr[j] = fr[j - 1]                                # shares its frame
            if k and L:
                u = rng.random()
                if u < 0.15:
                    fr[k - 1] = L - 1
                elif u < 0.22:
                    fr[k - 1] = L + rng.integers(0, 3)               # at or above out_len
            if k >= 2 and L and rng.random() < 0.03:
                fr[k - 2] = L + 1                                    # ... and one more impulse behind such a one
                fr[k - 1] = L + 1 + rng.integers(0, 2)
            per.append(fr)
        inst = np.concatenate([np.full(len(f), i, np.uint32) for i, f in enumerate(per)]) if per else np.zeros(0, np.uint32)
        frame = np.concatenate(per).astype(np.uint32) if per else np.zeros(0, np.uint32)
        keys = np.concatenate([np.sort(rng.random(len(f))) for f in per]) if per else np.zeros(0)
        order = np.argsort(keys, kind="stable")
        inst, frame = inst[order], frame[order]
        n = len(inst)
        rec = np.zeros(n, REC)
        rec["freq"] = rng.uniform(50, 2000, n)
        rec["on"] = rng.random(n) < 0.6
        rec["tag"] = np.arange(tag, tag + n)
        tag += n
        out.append((L, inst, frame, rng.integers(1, 7, n).astype(np.uint64), rec))
    return out


class HostLive:
    """The only live route without this bank: one ImpulseQueue, one PolyphonyDispatcher and P Triggers per instrument, called from the host."""

    def __init__(self, n_instruments, polyphony, rec_dtype=REC, note_on_offset=ON_OFFSET):
        self.lib = L = abi.load()
        self.n, self.P, self.dtype, self.W = n_instruments, polyphony, np.dtype(rec_dtype), np.dtype(rec_dtype).itemsize // 4
        self.on_word, self.on_shift = note_on_offset // 4, 8 * (note_on_offset % 4)
        size = self.dtype.itemsize
        self.queues, self.dispatchers, self.triggers = [], [], []
        for _ in range(n_instruments):
            q, d = C.c_void_p(), C.c_void_p()
            abi.check(L.zh_impulse_queue_create(size, C.byref(q)), "zh_impulse_queue_create")
            abi.check(L.zh_polyphony_dispatcher_create(polyphony, size, note_on_offset, C.byref(d)), "zh_polyphony_dispatcher_create")
            ts = []
            for _ in range(polyphony):
                t = C.c_void_p()
                abi.check(L.zh_trigger_create(size, C.byref(t)), "zh_trigger_create")
                ts.append(t)
            self.queues.append(q); self.dispatchers.append(d); self.triggers.append(ts)
        V = n_instruments * polyphony
        # derived state, in the shape of zh_voice_bank_live_get_state
        self.next_event_id = np.ones(n_instruments, np.uint64)
        self.slot = np.zeros(V, [("used", "u4"), ("note_on", "u4"), ("note_id", "u8"), ("event_id", "u8")])
        self.trig = np.zeros(V, [("has_note", "u4"), ("note_id", "u8"), ("carried", "u4", 16)])
        self.note_of_tag = {}
        self.stats = {"over_32": 0, "out_of_order_drops": 0, "steals_of_live_notes": 0, "lost_note_offs": 0, "longest_carry": 0, "spans": 0}
        self._carry = [(0, 0)] * V               # (tag the voice ended on, buffers it has been carried into)

    def _on(self, words):
        return ((int(words[self.on_word]) >> self.on_shift) & 0xff) != 0

    def schedule(self, out_len, inst, frame, note_id, rec, cap=ROWS):
        """one buffer -> tables shaped like the bank's (count [V], start / end [cap][V], words [W][cap][V], ...)"""
        L, P, V, Wn = self.lib, self.P, self.n * self.P, self.W
        out = {"count": np.zeros(V, np.uint32), "start": np.zeros((cap, V), np.uint32), "end": np.zeros((cap, V), np.uint32),
               "words": np.zeros((Wn, cap, V), np.uint32), "note_id_changed": np.zeros((cap, V), np.uint8)}
        rec = np.ascontiguousarray(rec, self.dtype)
        words = rec.view(np.uint32).reshape(len(rec), Wn)
        by_inst = [[] for _ in range(self.n)]
        for k in range(len(inst)):
            by_inst[int(inst[k])].append(k)
        iap, poly, ps = abi.Iap(), (abi.Iap * P)(), abi.PaintSpan()
        for i, ks in enumerate(by_inst):
            accepted = []                                            # ImpulseQueue's two rules, restated to count the drops
            if len(ks) > 32:
                self.stats["over_32"] += 1
            for k in ks:
                abi.check(L.zh_impulse_queue_push(self.queues[i], int(frame[k]), int(note_id[k]), rec[k:k + 1].ctypes.data), "zh_impulse_queue_push")
                if len(accepted) >= 32:
                    continue
                if accepted and frame[k] < frame[accepted[-1]]:
                    self.stats["out_of_order_drops"] += 1
                    continue
                accepted.append(k)
                if Wn > TAG_WORD:
                    self.note_of_tag[int(words[k][TAG_WORD])] = int(note_id[k])
            abi.check(L.zh_impulse_queue_consume(self.queues[i], C.byref(iap)), "zh_impulse_queue_consume")
            first_id = int(self.next_event_id[i])
            assert iap.len == len(accepted) and all(iap.impulses[j].event_id == first_id + j and iap.impulses[j].frame == frame[k]
                                                    for j, k in enumerate(accepted))
            self.next_event_id[i] += len(accepted)
            abi.check(L.zh_polyphony_dispatcher_dispatch(self.dispatchers[i], iap, poly), "zh_polyphony_dispatcher_dispatch")
            landed = []
            for s in range(P):
                for j in range(poly[s].len):
                    imp = poly[s].impulses[j]
                    landed.append((int(imp.event_id), s, int(imp.note_id)))
            for event_id, s, nid in sorted(landed):
                on = self._on(words[accepted[event_id - first_id]])
                sl = self.slot[i * P + s]
                if on and sl["used"] and sl["note_on"]:
                    self.stats["steals_of_live_notes"] += 1
                self.slot[i * P + s] = (1, 1 if on else 0, nid, event_id)
            got = {e for e, _, _ in landed}
            self.stats["lost_note_offs"] += sum(1 for j, k in enumerate(accepted) if first_id + j not in got and not self._on(words[k]))
            for s in range(P):
                v = i * P + s
                abi.check(L.zh_trigger_counter(self.triggers[i][s], 0, out_len, poly[s]), "zh_trigger_counter")
                n, tags = 0, []
                while True:
                    rc = L.zh_trigger_next(self.triggers[i][s], C.byref(ps))
                    assert rc >= 0
                    if rc == 0:
                        break
                    w = np.frombuffer(ps.params, np.uint32, Wn).copy()
                    assert n < cap
                    out["start"][n, v], out["end"][n, v], out["note_id_changed"][n, v] = ps.start, ps.end, ps.note_id_changed
                    out["words"][:, n, v] = w
                    n += 1
                    self.trig[v]["has_note"] = 1
                    self.trig[v]["carried"][:] = 0
                    self.trig[v]["carried"][:Wn] = w
                    if Wn > TAG_WORD:
                        tags.append(int(w[TAG_WORD]))
                        self.trig[v]["note_id"] = self.note_of_tag[tags[-1]]
                out["count"][v] = n
                self.stats["spans"] += n
                if tags:
                    last, run = self._carry[v]
                    run = run + 1 if tags[0] == last else 0
                    self.stats["longest_carry"] = max(self.stats["longest_carry"], run)
                    self._carry[v] = (tags[-1], run if tags[-1] == tags[0] else 0)
        out["note_on"] = (((out["words"][self.on_word] >> self.on_shift) & 0xff) != 0).astype(np.uint8)
        return out

    def reset(self):
        """what zh_voice_bank_reset does on a live bank: the dispatcher and the Triggers; ImpulseQueue has no reset"""
        for d in self.dispatchers:
            abi.check(self.lib.zh_polyphony_dispatcher_reset(d), "reset")
        for ts in self.triggers:
            for t in ts:
                abi.check(self.lib.zh_trigger_reset(t), "reset")
        self.slot[:] = 0
        self.trig[:] = 0

    def close(self):
        for q in self.queues:
            self.lib.zh_impulse_queue_destroy(q)
        for d in self.dispatchers:
            self.lib.zh_polyphony_dispatcher_destroy(d)
        for ts in self.triggers:
            for t in ts:
                self.lib.zh_trigger_destroy(t)
        self.queues, self.dispatchers, self.triggers = [], [], []


@functools.lru_cache(maxsize=None)
def reference(n_instruments, polyphony, seed=SEED, frames=FRAMES):
    """the corpus through HostLive, computed once per shape and shared: (tables per buffer, the HostLive with its final state and stats)"""
    host = HostLive(n_instruments, polyphony)
    tables = [host.schedule(*buf) for buf in corpus(n_instruments, seed, frames)]
    host.close()
    return tables, host


def assert_coverage(stats, n_buffers):
    """on the reference alone: the corpus reaches the paths the live lane steps add"""
    assert stats["over_32"] >= 1, stats
    assert stats["out_of_order_drops"] >= 1, stats
    assert stats["steals_of_live_notes"] >= 1, stats
    assert stats["lost_note_offs"] >= 1, stats
    assert stats["longest_carry"] >= 3, stats
    assert stats["spans"] > n_buffers, stats


def assert_state_equal(next_event_id, voices, host, what=""):
    """device state (LiveVoiceBank.get_state) against the reference's"""
    assert np.array_equal(np.asarray(next_event_id)[:host.n], host.next_event_id), (what, "next_event_id")
    for v in range(host.n * host.P):
        g, s, t = voices[v], host.slot[v], host.trig[v]
        assert bool(g.used) == bool(s["used"]), (what, v, "used")
        if s["used"]:
            assert (g.note_on, g.note_id, g.event_id) == (s["note_on"], s["note_id"], s["event_id"]), (what, v, "slot")
        assert bool(g.has_note) == bool(t["has_note"]), (what, v, "has_note")
        if t["has_note"]:
            assert g.trigger_note_id == t["note_id"] and list(g.carried) == list(t["carried"]), (what, v, "trigger")
