"""zangscript modules on the GPU: compile a script (the C++ front-end in libzang_hip.so), load its fused kernels
(zh_script_load -> hiprtc) and paint them through the module call shape of the reference
(SineOsc.zig:22-31; generated modules: codegen_zig.zig:558-563)."""
import ctypes as C
import os

import numpy as np
import torch

from . import abi, zscript_native as native
from .runtime import as_bool, as_buf, default_context


class ScriptCompileError(Exception):
    pass


class HipBackendError(Exception):
    """The script compiled, but this module uses something the HIP backend does not generate (the message says what)."""


def compile_hip(hip_source):
    """hiprtc compile only (works without a GPU); returns the gfx950 code object's size."""
    lib = abi.load()
    code, n = C.c_void_p(), C.c_size_t()
    log = C.create_string_buffer(1 << 16)
    rc = lib.zh_script_compile(hip_source.encode(), C.byref(code), C.byref(n), log, len(log))
    if rc != 0:
        raise ScriptCompileError("hiprtc failed (%d):\n%s" % (rc, log.value.decode(errors="replace")))
    lib.zh_script_free_code(code)
    return n.value


class ScriptProgram:
    """One script: front-end result + the loaded hipModule."""

    def __init__(self, text, ctx=None, filename="script.txt", only=None, forms=native.FORM_ROLES_WORTH, hip_patch=None, code_cache=None, spans=False):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.text, self.filename = text, filename
        try:                                                    # the C++ compiler in libzang_hip.so (zh_zscript_*)
            compiled = native.NativeScript(text, filename)
        except native.NativeScriptError as e:
            raise ScriptCompileError(str(e))
        # ZH_SCRIPT_UNROLL: frames per unrolled chunk of the generated kernels (an experiment knob; 0 / unset = the emitter's choice by body size)
        # forms: FORM_ROLES_WORTH = modules the emitter expects to gain from it also as a role-wave kernel for few voices (zs_paint_pc_<name>;
        # the library picks per paint); FORM_ROLES = every module (the parity tests force the form)
        forms = int(os.environ.get("ZH_SCRIPT_FORMS", forms))       # (an experiment knob like ZH_SCRIPT_UNROLL)
        # spans=True: also zs_paint_spans_<name> (ScriptModule.paint_spans) -- one more hiprtc kernel per module, so not by default
        if spans:
            forms |= native.FORM_SPANS
        self.hip_source, self.meta = compiled.generate_hip(only=only, unroll=int(os.environ.get("ZH_SCRIPT_UNROLL", "0")), forms=forms)
        if hip_patch is not None:                               # experiments (tools/exp/role_probe.py): the generated text, edited
            self.hip_source = hip_patch(self.hip_source)
        h = C.c_void_p()
        log = C.create_string_buffer(1 << 16)
        # code_cache = a directory: the compiled code object is kept there under the hash of the generated text (+ the library's version)
        # and loaded with zh_script_load_code next time -- the reference's compile-once flow; hiprtc takes 1-4 s per module
        self.loaded_from_cache = False
        cache_file = None
        if code_cache is not None and hip_patch is None:
            import hashlib
            key = hashlib.sha256(self.hip_source.encode() + b"\0" + self.lib.zh_version()).hexdigest()[:32]
            cache_file = os.path.join(code_cache, "zs_%s.hsaco" % key)
            if os.path.exists(cache_file):
                blob = open(cache_file, "rb").read()
                if self.lib.zh_script_load_code(self.ctx.handle, blob, len(blob), C.byref(h)) == 0:
                    compiled.close()
                    self.handle, self._modules, self.loaded_from_cache = h, [], True
                    self.ctx._children.add(self)
                    return
        if cache_file is not None:
            code, n = C.c_void_p(), C.c_size_t()
            if self.lib.zh_script_compile(self.hip_source.encode(), C.byref(code), C.byref(n), log, len(log)) == 0:
                blob = C.string_at(code, n.value)
                self.lib.zh_script_free_code(code)
                os.makedirs(code_cache, exist_ok=True)
                tmp = cache_file + ".%d.tmp" % os.getpid()
                open(tmp, "wb").write(blob)
                os.replace(tmp, cache_file)
                if self.lib.zh_script_load_code(self.ctx.handle, blob, len(blob), C.byref(h)) == 0:
                    compiled.close()
                    self.handle, self._modules = h, []
                    self.ctx._children.add(self)
                    return
        rc = self.lib.zh_script_load(self.ctx.handle, self.hip_source.encode(), C.byref(h), log, len(log))
        if rc != 0 and forms and hip_patch is None:
            # the lane kernels alone: a role-wave kernel hiprtc refuses must not take the patch away (none has been seen to)
            self.role_form_error = log.value.decode(errors="replace")
            self.hip_source, self.meta = compiled.generate_hip(only=only, unroll=int(os.environ.get("ZH_SCRIPT_UNROLL", "0")), forms=forms & native.FORM_SPANS)
            rc = self.lib.zh_script_load(self.ctx.handle, self.hip_source.encode(), C.byref(h), log, len(log))
        compiled.close()
        if rc != 0:
            raise ScriptCompileError("zh_script_load failed (%d):\n%s" % (rc, log.value.decode(errors="replace")))
        self.handle = h
        self._modules = []
        self.ctx._children.add(self)

    def module(self, name, n_voices, first_seed=0):
        m = self.meta.get(name)
        if m is None:
            raise KeyError("script exports no module named %r" % name)
        if "error" in m:
            raise HipBackendError("%s: %s" % (name, m["error"]))
        return ScriptModule(self, name, n_voices, first_seed)

    def close(self):
        if self.handle:
            for m in list(self._modules):
                m.close()
            self.lib.zh_script_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ENUM_LABELS = native.ENUM_LABELS


class ScriptModule:
    """n_voices instances of one exported script module.  num_outputs = 1; the temps the generated Zig
    would need live in registers, so `temps` is accepted and ignored."""
    num_outputs = 1

    def __init__(self, program, name, n_voices, first_seed=0):
        self.program, self.name, self.n = program, name, n_voices
        self.meta = program.meta[name]
        self.params = self.meta["params"]            # [(name, kind, enum name)], sample_rate first
        self.lib = program.lib
        h = C.c_void_p()
        abi.check(self.lib.zh_script_module_create(program.handle, name.encode(), n_voices, self.meta["state_words"],
                                                   first_seed, C.byref(h)), "zh_script_module_create")
        self.handle = h
        program._modules.append(self)

    @property
    def num_temps(self):
        """What the generated Zig struct would ask for (codegen_zig.zig:518); the fused kernel needs none."""
        return self.meta["num_temps"]

    def _param(self, kind, enum, value, keep):
        p = abi.ScriptParam()
        dev = self.program.ctx.device
        if kind == "constant":
            p.kind = abi.SP_CONSTANT
            if torch.is_tensor(value):
                assert value.dtype == torch.float32 and value.numel() == self.n and value.is_contiguous()
                p.pf = value.data_ptr(); keep.append(value)
            else:
                p.f = float(value)
        elif kind == "boolean":
            p.kind = abi.SP_BOOLEAN
            if torch.is_tensor(value):
                assert value.dtype == torch.uint8 and value.numel() == self.n and value.is_contiguous()
                p.pb = value.data_ptr(); keep.append(value)
            else:
                p.u = 1 if value else 0
        elif kind in ("constant_or_buffer", "buffer"):
            p.kind = abi.SP_COB if kind == "constant_or_buffer" else abi.SP_BUFFER
            if isinstance(value, abi.Cob):                      # zang.constant(...) / zang.buffer(...)
                keep.append(value)
                if value.tag == abi.COB_BUFFER:
                    p.is_buffer, p.pf, p.stride = 1, value.buffer.ptr, value.buffer.stride
                else:
                    p.f, p.pf = value.constant.value, value.constant.per_voice
            elif torch.is_tensor(value) and value.dim() == 2:
                b = as_buf(value); keep.append(value)
                p.is_buffer, p.pf, p.stride = 1, b.ptr, b.stride
            elif torch.is_tensor(value):
                assert kind == "constant_or_buffer" and value.dtype == torch.float32 and value.numel() == self.n
                p.pf = value.data_ptr(); keep.append(value)
            else:
                assert kind == "constant_or_buffer", "a waveform param needs a [frames, voices] image"
                p.f = float(value)
        elif kind == "curve":
            p.kind = abi.SP_CURVE
            if torch.is_tensor(value):                          # device array of (value, t) pairs
                p.pf, p.u = value.data_ptr(), value.numel() // 2; keep.append(value)
            else:                                               # [(t, value), ...] like a defcurve block
                nodes = np.array([(v, t) for t, v in value], np.float32).reshape(-1)
                tns = torch.from_numpy(nodes).to(dev)
                p.pf, p.u = tns.data_ptr(), len(value); keep.append(tns)
        else:                                                   # one_of
            p.kind = abi.SP_ENUM
            if isinstance(value, abi.Curve):                    # the library's own zang.PaintCurve.* values
                if enum != "PaintCurve":
                    raise TypeError("a PaintCurve value for a %s param" % enum)
                if value.duration.per_voice:
                    raise ValueError("a script module takes one PaintCurve duration for all voices, not a per-voice array")
                p.u, p.f = value.tag, value.duration.value
            else:                                               # ".label" or (".label", payload)
                label, payload = (value, None) if isinstance(value, str) else value
                p.u = _ENUM_LABELS[enum].index(label.lstrip("."))
                p.f = float(payload) if payload is not None else 0.0
        return p

    def _params(self, params, keep, defaults=()):
        arr = (abi.ScriptParam * abi.SCRIPT_MAX_PARAMS)()
        for i, (name, kind, enum) in enumerate(self.params):
            if name in params:
                arr[i] = self._param(kind, enum, params[name], keep)
            elif name in defaults:
                arr[i] = self._param(kind, enum, _default_value(kind, enum), keep)
            else:
                raise KeyError("missing param %r" % name)
        extra = set(params) - {n for n, _, _ in self.params}
        if extra:
            raise KeyError("module %s has no param(s) %s" % (self.name, sorted(extra)))
        return arr

    def paint_spans(self, span, outputs, table, params, zero_first=False):
        """The reference's Trigger loop for every voice in one launch (zh_script_module_paint_spans): voice v runs paint(sub-span k,
        ..., note_id_changed[k][v], params with the table's per-sub-span values) for each of its sub-spans in `table` (a
        ScriptSpanTable).  `params`: the dict paint() takes, for everything the table does not set (a param the table holds an
        array for may be left out).  Frames outside a voice's sub-spans are left alone, or zeroed with zero_first=True.  The
        program must be built with ScriptProgram(..., spans=True)."""
        abi.check(self._paint_spans(span, outputs, table, params, abi.PAINT_ZERO_FIRST if zero_first else 0), "zh_script_module_paint_spans")

    def _paint_spans(self, span, outputs, table, params, flags, span_params=None):
        """-> the return code; `span_params`: a ctypes ScriptSpanParam array to pass instead of the table's (the error tests)"""
        keep = []
        params = dict(params)
        params.update(table.constants)
        arr = self._params(params, keep, defaults=table.arrays)
        tb, sp = table.device(self.program.ctx.device, [p[0] for p in self.params])
        if span_params is not None:
            sp = span_params
        ob = as_buf(outputs[0])
        rc = self.lib.zh_script_module_paint_spans(self.handle, span.start, span.end, C.byref(ob), arr, len(self.params), sp, C.byref(tb), flags)
        self._keep = (keep, outputs, table)
        return rc

    def paint(self, span, outputs, temps, note_id_changed, params, zero_first=False, tolerant=False):
        """params: dict by name (sample_rate included), like the reference's Params struct literal.
        tolerant=True: ZH_PAINT_TOLERANT -- the module's sines that reach the output through scaling and adding alone (not another
        oscillator's freq / phase, a distortion, a divisor ...: csrc/zscript_emit.hip) are evaluated in f32; all state that is not a
        Filter's or a delay ring's stays exact."""
        keep = []
        arr = self._params(params, keep)
        ob = as_buf(outputs[0])
        nic = as_bool(note_id_changed)
        flags = (abi.PAINT_ZERO_FIRST if zero_first else 0) | (abi.PAINT_TOLERANT if tolerant else 0)
        abi.check(self.lib.zh_script_module_paint(self.handle, span.start, span.end, C.byref(ob), nic, arr, len(self.params), flags),
                  "zh_script_module_paint")
        self._keep = (keep, outputs, note_id_changed)

    @property
    def frame_ranges_ok(self):
        """True when the library may launch this module's kernel as frame ranges at small voice counts (no delay ring)."""
        return bool(self.lib.zh_script_module_ranges_ok(self.handle))

    def get_state(self):
        a = np.zeros((self.meta["state_words"], self.n), np.uint32)
        abi.check(self.lib.zh_script_module_get_state(self.handle, a.ctypes.data_as(C.c_void_p)), "zh_script_module_get_state")
        return a

    def set_state(self, a):
        a = np.ascontiguousarray(a, np.uint32)
        assert a.shape == (self.meta["state_words"], self.n)
        abi.check(self.lib.zh_script_module_set_state(self.handle, a.ctypes.data_as(C.c_void_p)), "zh_script_module_set_state")

    def close(self):
        if self.handle:
            self.lib.zh_script_module_destroy(self.handle)
            self.handle = None
            if self in self.program._modules:
                self.program._modules.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _default_value(kind, enum):
    if kind == "boolean":
        return False
    if kind == "one_of":
        return _ENUM_LABELS[enum][0]
    return 0.0


def _span_value(kind, enum, value):
    """a per-sub-span value as the span arrays hold it: (f, u)"""
    if kind in ("constant", "constant_or_buffer"):
        return float(np.float32(value)), None
    if kind == "boolean":
        return None, 1 if value else 0
    if kind == "one_of":
        label, payload = (value, None) if isinstance(value, str) else value
        return float(np.float32(payload if payload is not None else 0.0)), _ENUM_LABELS[enum].index(label.lstrip("."))
    raise ValueError("a %s param can not vary per sub-span" % kind)


class ScriptSpanTable:
    """Per-voice sub-spans of one buffer for ScriptModule.paint_spans (zh_script_span_table): count [V], start / end /
    note_id_changed [K][V], and per-sub-span values of params ([K][V] arrays: `f` float32 for a constant, a cob's constant or an
    enum's payload, `u` uint32 for a boolean or an enum's index).  Host arrays (numpy); paint_spans uploads them once.
    `spec`: the module's params [(name, kind, enum name)] (ScriptModule.params, or the meta of ScriptProgram / NativeScript)."""

    def __init__(self, spec, count, start, end, note_id_changed, values=None, constants=None):
        self.spec = list(spec)
        self.count = np.ascontiguousarray(count, np.uint32)
        V = len(self.count)
        self.start = np.ascontiguousarray(start, np.uint32).reshape(-1, V)
        self.end = np.ascontiguousarray(end, np.uint32).reshape(-1, V)
        self.note_id_changed = np.ascontiguousarray(note_id_changed, np.uint8).reshape(-1, V)
        self.max_spans = self.start.shape[0]
        assert self.max_spans >= 1 and self.end.shape == self.start.shape == self.note_id_changed.shape
        kinds = {n: (k, e) for n, k, e in self.spec}
        self.arrays = {}                                     # name -> (f [K][V] float32 or None, u [K][V] uint32 or None)
        for name, (f, u) in (values or {}).items():
            if name not in kinds:
                raise KeyError("no param %r" % name)
            self.arrays[name] = (None if f is None else np.ascontiguousarray(f, np.float32).reshape(self.max_spans, V),
                                 None if u is None else np.ascontiguousarray(u, np.uint32).reshape(self.max_spans, V))
        self.constants = dict(constants or {})              # name -> a value every sub-span shares (set on the paint's params)
        self._dev = None

    @property
    def n_voices(self):
        return len(self.count)

    @classmethod
    def from_lists(cls, spec, per_voice, max_spans=None):
        """per_voice[v] = [(start, end, note_id_changed, {param: value}), ...] in the order the voice paints them -- a value as
        paint() takes it (a float, a bool, ".label" or (".label", payload)).  A param whose value is the same in every sub-span
        gets no array."""
        V = len(per_voice)
        K = max_spans or max([len(x) for x in per_voice] + [1])
        count = np.array([min(len(x), K) for x in per_voice], np.uint32)
        start = np.zeros((K, V), np.uint32); end = np.zeros((K, V), np.uint32); nic = np.zeros((K, V), np.uint8)
        kinds = {n: (k, e) for n, k, e in spec}
        seen = {}
        for v, spans in enumerate(per_voice):
            for k, (s, e, n, vals) in enumerate(spans[:K]):
                start[k, v], end[k, v], nic[k, v] = s, e, 1 if n else 0
                for name, value in vals.items():
                    if name not in kinds:
                        raise KeyError("no param %r" % name)
                    seen.setdefault(name, {})[(k, v)] = _span_value(kinds[name][0], kinds[name][1], value)
        values, constants = {}, {}
        for name, cells in seen.items():
            distinct = set(cells.values())
            total = int(count.sum())
            if len(distinct) == 1 and len(cells) == total:
                f, u = next(iter(distinct))
                kind, enum = kinds[name]
                if kind == "boolean":
                    constants[name] = bool(u)
                elif kind == "one_of":
                    constants[name] = (_ENUM_LABELS[enum][u], f)
                else:
                    constants[name] = f
                continue
            fa = np.zeros((K, V), np.float32); ua = np.zeros((K, V), np.uint32)
            has_f = has_u = False
            for (k, v), (f, u) in cells.items():
                if f is not None:
                    fa[k, v] = f; has_f = True
                if u is not None:
                    ua[k, v] = u; has_u = True
            values[name] = (fa if has_f else None, ua if has_u else None)
        return cls(spec, count, start, end, nic, values, constants)

    def device(self, dev, order):
        """-> (zh_script_span_table, zh_script_span_param array in the module's param order); uploads once"""
        if self._dev is None:
            def up(a):
                return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
            keep = [up(self.count), up(self.start), up(self.end), up(self.note_id_changed)]
            arrays = {}
            for name, (f, u) in self.arrays.items():
                tf = up(f) if f is not None else None
                tu = up(u) if u is not None else None
                keep += [t for t in (tf, tu) if t is not None]
                arrays[name] = (tf, tu)
            self._dev = (keep, arrays)
        keep, arrays = self._dev
        tb = abi.ScriptSpanTable(self.max_spans, 0, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
        sp = (abi.ScriptSpanParam * abi.SCRIPT_MAX_PARAMS)()
        for i, name in enumerate(order):
            if name in arrays:
                tf, tu = arrays[name]
                sp[i] = abi.ScriptSpanParam(tf.data_ptr() if tf is not None else None, tu.data_ptr() if tu is not None else None)
        return tb, sp


class PolyScriptVoice:
    """example_script_runtime_poly.zig's MainModule.paint, offline: the notes of `events` go through NoteTracker ->
    PolyphonyDispatcher(polyphony) -> one Trigger per sub-voice (zh_poly_voice), and the sub-spans of a buffer with their note
    params become one ScriptSpanTable for `module` (a ScriptModule of `polyphony` voices): one paint_spans per buffer.
    `note_params`: the module's params a note carries (constant / cob / boolean; `note_on` among them);
    `events`: [(t seconds, note id, {param: value})]."""

    def __init__(self, module, polyphony, note_params, events, device=False):
        """device=True: the tables are filled on the device by a voice bank (zang_amd.bank) on the module's context and never
        leave it -- the same bits, no host scheduling or upload per buffer; spans then start at frame 0."""
        assert module.n == polyphony
        self.module, self.polyphony = module, polyphony
        kinds = {n: k for n, k, _ in module.params}
        self.note_params = list(note_params)
        for n in self.note_params:
            if kinds.get(n) not in ("constant", "constant_or_buffer", "boolean"):
                raise ValueError("note param %r: a constant, cob or boolean param of the module" % n)
        if "note_on" not in self.note_params:
            raise ValueError("the notes must carry note_on (PolyphonyDispatcher reads it)")
        self.kinds = [kinds[n] for n in self.note_params]
        # the note record zh_poly_voice copies about: one 4-byte slot per param (f32, or a bool in its first byte)
        self.dtype = np.dtype({"names": self.note_params, "formats": ["<f4" if k != "boolean" else "u1" for k in self.kinds],
                               "offsets": [4 * j for j in range(len(self.note_params))], "itemsize": 4 * len(self.note_params)})
        rec = np.zeros(max(len(events), 1), self.dtype)
        for i, (_, _, vals) in enumerate(events):
            for n in self.note_params:
                rec[i][n] = vals[n]
        t = np.array([e[0] for e in events], np.float32)
        ids = np.array([e[1] for e in events], np.uint64)
        self._rec = rec
        self.lib = module.lib
        self.bank = None
        self.handle = None
        if device:
            from .bank import VoiceBank
            self.bank = VoiceBank(module.program.ctx, polyphony, rec[:len(events)], [0, len(events)], t, ids, 4 * self.note_params.index("note_on"), rows=34)
            return
        h = C.c_void_p()
        abi.check(self.lib.zh_poly_voice_create(polyphony, self.dtype.itemsize, 4 * self.note_params.index("note_on"), len(events),
                                                rec.ctypes.data, t.ctypes.data, ids.ctypes.data, C.byref(h)), "zh_poly_voice_create")
        self.handle = h

    def schedule(self, frames, sample_rate):
        """the next buffer's sub-spans (frames [0, frames)) as a ScriptSpanTable"""
        P = self.polyphony
        cap = 34                                            # <= 32 impulses + carry-over per sub-voice and buffer
        if self.bank is not None:
            self.bank.schedule([frames], sample_rate, cap)
            return self.bank.script_table(cap, {n: (j, "u" if k == "boolean" else "f") for j, (n, k) in enumerate(zip(self.note_params, self.kinds))})
        count = np.zeros(P, np.uint32)
        start = np.zeros((cap, P), np.uint32); end = np.zeros((cap, P), np.uint32)
        rec = np.zeros((cap, P), self.dtype); nic = np.zeros((cap, P), np.uint8)
        fr = np.array([frames], np.uint32)
        abi.check(self.lib.zh_poly_voice_schedule(self.handle, float(sample_rate), fr.ctypes.data, 1, cap, count.ctypes.data, start.ctypes.data,
                                                  end.ctypes.data, rec.ctypes.data, nic.ctypes.data), "zh_poly_voice_schedule")
        K = max(int(count.max()), 1)
        values = {}
        for n, k in zip(self.note_params, self.kinds):
            values[n] = (None, rec[n][:K].astype(np.uint32)) if k == "boolean" else (np.ascontiguousarray(rec[n][:K]), None)
        return ScriptSpanTable(self.module.params, count, start[:K], end[:K], nic[:K], values)

    def paint(self, span, outputs, params, sample_rate):
        """one buffer: schedule it, then one paint_spans with zero_first (frames no note covers are zero).  Returns the table."""
        if self.bank is not None and span.start:
            raise ValueError("a device-scheduled voice paints spans that start at frame 0")
        table = self.schedule(span.end - span.start, sample_rate)
        if span.start:
            table.start += np.uint32(span.start); table.end += np.uint32(span.start)
        self.module.paint_spans(span, outputs, table, params, zero_first=True)
        return table

    def close(self):
        if self.bank is not None:
            self.bank.close()
            self.bank = None
        if self.handle:
            self.lib.zh_poly_voice_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
