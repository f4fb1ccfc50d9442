"""What the stages that fill a [span][player] table share on the Python side (csrc/span_stage.hip.h is the native half): the view a
span paint takes, and the stage's reserve / overflows / script_table / download / close over the C functions of one prefix."""
import ctypes as C

import numpy as np

from . import abi


class SpanTableView:
    """What a span paint takes (zh_script_span_table + zh_script_span_param): .tb, and .arrays by param name.  No copy."""

    def device(self, dev, order):
        sp = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
        for i, name in enumerate(order):
            if name in self.arrays:
                sp[i] = self.arrays[name]
        return self.tb, sp


class StageTable(SpanTableView):
    """A view of a stage's table; `fields`: (name, field index) of the arrays it hands out."""

    def __init__(self, stage, max_spans, fields):
        self.stage, self.max_spans, self.n_voices = stage, max_spans, stage.n_players
        self.tb = abi.ScriptSpanTable()
        stage._call("script_table", max_spans, C.byref(self.tb))
        self.arrays = {}
        for name, field in fields:
            self.arrays[name] = sp = abi.ScriptSpanParam()
            stage._call("span_param", field, C.byref(sp))


class Stage:
    """The base of ArpStage, SubsongStage and SpanMerge.  A subclass sets PREFIX (its C functions are PREFIX_reserve, ...) and
    FIELDS, the (name, field index) list of its table (SpanMerge: per instance); its __init__ creates the handle through _create."""

    def _create(self, ctx, n_players, rows, *args):
        self.ctx, self.lib, self.n_players = ctx, ctx.lib, int(n_players)
        self.handle = C.c_void_p()
        abi.check(getattr(self.lib, f"{self.PREFIX}_create")(ctx.handle, self.n_players, *args, C.byref(self.handle)), f"{self.PREFIX}_create")
        ctx._children.add(self)
        if rows is not None:
            self.reserve(rows)

    def _call(self, name, *args):
        fn = f"{self.PREFIX}_{name}"
        abi.check(getattr(self.lib, fn)(self.handle, *args), fn)

    def reserve(self, rows):
        """table capacity in rows; invalidates views and graphs made before it"""
        self._call("reserve", rows)

    def script_table(self, max_spans):
        return StageTable(self, max_spans, self.FIELDS)

    def overflows(self):
        """rows dropped so far because a player's list was full (synchronises)"""
        n = C.c_uint64()
        self._call("overflows", C.byref(n))
        return n.value

    def download(self, max_spans, dtypes=None):
        """the stage's table as host arrays (synchronises; for tests and debugging): count [N], start / end [K][N] uint32, nic
        [K][N] uint8, and every field by name, [K][N] uint32 (the words of an "f" field as bits) unless `dtypes` names another.
        Rows at or above a player's count hold whatever was there."""
        N, K = self.n_players, max_spans
        t = self.script_table(K)

        def down(ptr, shape, dtype):
            a = np.zeros(shape, dtype)
            if a.size:
                abi.check(self.lib.zh_download(self.ctx.handle, a.ctypes.data, ptr, a.nbytes), "zh_download")
            return a
        out = {"count": down(t.tb.count, (N,), np.uint32), "start": down(t.tb.start, (K, N), np.uint32), "end": down(t.tb.end, (K, N), np.uint32),
               "nic": down(t.tb.note_id_changed, (K, N), np.uint8)}
        for name, sp in t.arrays.items():
            out[name] = down(sp.f or sp.u, (K, N), (dtypes or {}).get(name, np.uint32))
        return out

    def close(self):
        if self.handle:
            getattr(self.lib, f"{self.PREFIX}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass
