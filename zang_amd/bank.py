"""Voice bank: N instruments' NoteTracker -> PolyphonyDispatcher -> Trigger scheduling on the device
(zh_voice_bank_*, csrc/sched_bank.hip).  One launch per call fills the [span][voice] tables the *_paint_spans entry points
read; the views below hand those tables to the paints as device pointers, without a copy."""
import ctypes as C

import numpy as np

from . import abi
from .stage import SpanTableView


class BankSpanTable:
    """What NiceInstrument / PMOscInstrument.paint_spans take (zh_span_table): a view of the bank's tables."""

    def __init__(self, bank, max_spans, freq_word):
        self.bank, self.max_spans = bank, max_spans
        self.c = abi.SpanTable()
        abi.check(bank.lib.zh_voice_bank_span_table(bank.handle, max_spans, freq_word, C.byref(self.c)), "zh_voice_bank_span_table")


class BankScriptTable(SpanTableView):
    """What ScriptModule.paint_spans and the builtin modules' paint_spans take (zh_script_span_table + zh_script_span_param): a
    view of the bank's tables.  `fields`: {param name: (record word, "f" or "u")} -- "u" for a boolean (its byte first in an
    otherwise zero word) or an enum's index; `constants`: {param name: value} shared by every sub-span."""

    def __init__(self, bank, max_spans, fields, constants=None):
        self.bank, self.max_spans = bank, max_spans
        self.n_voices = bank.n_voices
        self.constants = dict(constants or {})
        self.tb = abi.ScriptSpanTable()
        abi.check(bank.lib.zh_voice_bank_script_table(bank.handle, max_spans, C.byref(self.tb)), "zh_voice_bank_script_table")
        self.arrays = {}
        for name, (word, view) in fields.items():
            sp = abi.ScriptSpanParam()
            abi.check(bank.lib.zh_voice_bank_span_param(bank.handle, word, C.byref(sp)), "zh_voice_bank_span_param")
            self.arrays[name] = abi.ScriptSpanParam(sp.f if view == "f" else None, sp.u if view == "u" else None)


class VoiceBank:
    """n instruments of one polyphony.  `records`: a numpy structured array (one record per event, itemsize a multiple of 4,
    at most 64 bytes); `offsets` [n + 1]: instrument i owns events [offsets[i], offsets[i + 1]) of records / t / note_ids;
    `note_on_offset`: the byte of a record that holds note_on.  `rows`: table capacity (max_spans may not exceed it)."""

    def __init__(self, ctx, polyphony, records, offsets, t, note_ids, note_on_offset, rows=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.polyphony = polyphony
        offsets = np.ascontiguousarray(offsets, np.uint64)
        self.n_instruments = max(len(offsets) - 1, 0)
        self.n_voices = self.n_instruments * polyphony
        records = np.ascontiguousarray(records)
        t = np.ascontiguousarray(t, np.float32)
        note_ids = np.ascontiguousarray(note_ids, np.uint64)
        self.params_size = records.dtype.itemsize
        self.handle = C.c_void_p()
        abi.check(self.lib.zh_voice_bank_create(ctx.handle, self.n_instruments, polyphony, self.params_size, note_on_offset,
                                                offsets.ctypes.data if self.n_instruments else None, records.ctypes.data, t.ctypes.data,
                                                note_ids.ctypes.data, C.byref(self.handle)), "zh_voice_bank_create")
        ctx._children.add(self)
        if rows is not None:
            self.reserve(rows)

    def reserve(self, rows):
        """table capacity in rows; invalidates views and graphs made before it"""
        abi.check(self.lib.zh_voice_bank_reserve(self.handle, rows), "zh_voice_bank_reserve")

    def reset(self):
        abi.check(self.lib.zh_voice_bank_reset(self.handle), "zh_voice_bank_reset")

    def schedule(self, frames, sample_rate, max_spans):
        """advance every instrument by the buffers of `frames` (an int or a list) and fill the tables: enqueued, no sync"""
        fr = np.atleast_1d(np.asarray(frames, np.uint32))
        abi.check(self.lib.zh_voice_bank_schedule(self.handle, float(sample_rate), fr.ctypes.data, len(fr), max_spans), "zh_voice_bank_schedule")

    def span_table(self, max_spans, freq_word=0):
        return BankSpanTable(self, max_spans, freq_word)

    def script_table(self, max_spans, fields, constants=None):
        return BankScriptTable(self, max_spans, fields, constants)

    def overflows(self):
        """sub-spans dropped so far because a voice's list was full (synchronises)"""
        n = C.c_uint64()
        abi.check(self.lib.zh_voice_bank_overflows(self.handle, C.byref(n)), "zh_voice_bank_overflows")
        return n.value

    def download(self, max_spans):
        """the tables as host arrays (synchronises; for tests and debugging): count [V], start / end [K][V], words [W][K][V]
        uint32, note_on / note_id_changed [K][V] uint8.  Rows at or above a voice's count hold whatever was there."""
        V, K, W = self.n_voices, max_spans, self.params_size // 4
        tb = self.span_table(K, 0).c

        def down(ptr, shape, dtype):
            a = np.zeros(shape, dtype)
            if a.size:
                abi.check(self.lib.zh_download(self.ctx.handle, a.ctypes.data, ptr, a.nbytes), "zh_download")
            return a
        words = np.zeros((W, K, V), np.uint32)
        for w in range(W):
            sp = abi.ScriptSpanParam()
            abi.check(self.lib.zh_voice_bank_span_param(self.handle, w, C.byref(sp)), "zh_voice_bank_span_param")
            words[w] = down(sp.u, (K, V), np.uint32)
        return {"count": down(tb.count, (V,), np.uint32), "start": down(tb.start, (K, V), np.uint32), "end": down(tb.end, (K, V), np.uint32),
                "words": words, "note_on": down(tb.note_on, (K, V), np.uint8), "note_id_changed": down(tb.note_id_changed, (K, V), np.uint8)}

    def get_state(self):
        inst = (abi.VoiceBankInstrumentState * max(self.n_instruments, 1))()
        voices = (abi.VoiceBankVoiceState * max(self.n_voices, 1))()
        abi.check(self.lib.zh_voice_bank_get_state(self.handle, inst, voices), "zh_voice_bank_get_state")
        return inst, voices

    def set_state(self, state):
        abi.check(self.lib.zh_voice_bank_set_state(self.handle, state[0], state[1]), "zh_voice_bank_set_state")

    def close(self):
        if self.handle:
            self.lib.zh_voice_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


class LiveVoiceBank(VoiceBank):
    """A bank without a song (zh_voice_bank_create_live): impulses are pushed from outside, as into the reference's ImpulseQueue, and
    every schedule() call takes what was pushed since the last one through ImpulseQueue -> PolyphonyDispatcher -> Triggers for one
    buffer, in one kernel.  `record_dtype`: the note params as a numpy structured dtype (itemsize a multiple of 4, at most 64);
    `max_impulses`: the most pushes one schedule() may carry.  Views, reserve, reset, overflows, download and close as on VoiceBank."""

    def __init__(self, ctx, n_instruments, polyphony, record_dtype, note_on_offset, max_impulses, rows=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.polyphony, self.n_instruments = polyphony, n_instruments
        self.n_voices = n_instruments * polyphony
        self.record_dtype = np.dtype(record_dtype)
        self.params_size = self.record_dtype.itemsize
        self.max_impulses = max_impulses
        self._pushed = ([], [], [], [])
        self.handle = C.c_void_p()
        abi.check(self.lib.zh_voice_bank_create_live(ctx.handle, n_instruments, polyphony, self.params_size, note_on_offset, max_impulses,
                                                     C.byref(self.handle)), "zh_voice_bank_create_live")
        ctx._children.add(self)
        if rows is not None:
            self.reserve(rows)

    def push(self, instrument, frame, note_id, record):
        """ImpulseQueue.push for one instrument (scalars), or for many at once (equal-length arrays, in push order)"""
        for acc, x in zip(self._pushed, (np.atleast_1d(np.asarray(instrument, np.uint32)), np.atleast_1d(np.asarray(frame, np.uint32)),
                                         np.atleast_1d(np.asarray(note_id, np.uint64)), np.atleast_1d(np.asarray(record, self.record_dtype)))):
            acc.append(x)
        if not len(self._pushed[0][-1]) == len(self._pushed[1][-1]) == len(self._pushed[2][-1]) == len(self._pushed[3][-1]):
            for acc in self._pushed:
                acc.pop()
            raise ValueError("push: instrument, frame, note_id and record differ in length")

    def schedule(self, out_len, max_spans):
        """one buffer of out_len frames from what was pushed since the last call: enqueued, no sync"""
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros(0, dt)
        inst, frame, ids, rec = (cat(xs, dt) for xs, dt in zip(self._pushed, (np.uint32, np.uint32, np.uint64, self.record_dtype)))
        self._pushed = ([], [], [], [])
        batch = abi.BankImpulses(len(inst), inst.ctypes.data, frame.ctypes.data, ids.ctypes.data, rec.ctypes.data)
        abi.check(self.lib.zh_voice_bank_schedule_live(self.handle, out_len, max_spans, C.byref(batch) if len(inst) else None),
                  "zh_voice_bank_schedule_live")

    def get_state(self):
        """(next_event_id [n] uint64, per-voice zh_voice_bank_live_voice_state array)"""
        next_id = np.zeros(max(self.n_instruments, 1), np.uint64)
        voices = (abi.VoiceBankLiveVoiceState * max(self.n_voices, 1))()
        abi.check(self.lib.zh_voice_bank_live_get_state(self.handle, next_id.ctypes.data_as(C.POINTER(C.c_uint64)), voices), "zh_voice_bank_live_get_state")
        return next_id, voices

    def set_state(self, state):
        next_id = np.ascontiguousarray(state[0], np.uint64)
        abi.check(self.lib.zh_voice_bank_live_set_state(self.handle, next_id.ctypes.data_as(C.POINTER(C.c_uint64)), state[1]), "zh_voice_bank_live_set_state")
