"""A restatement of examples/example_fmsynth.zig:22-356 (decibels, Oscillator, Operator, Instrument) in np.float32, vectorised
over voices and sequential over frames -- the yardstick of the FM tests; it holds no tests itself.  Every sine and pow comes
from the oracle (zo_math_sinf_n, zo_math_powf), every envelope from zo_envelope_paint, and the buffer operations (zero,
multiplyScalar, addScalarInto, multiplyWithScalar, multiplyWith, multiply) are written as the rounded f32 operations they are.
tests/test_fm_reference.py pins this file to the committed oracle.

Besides Instrument.paint it runs the Trigger loop per voice from a span table (:457-496), composes MainModule (:358-497) from
the host classes of zang_amd/notes.py, and counts per operator how many sine arguments fell into each of musl's classes."""
import ctypes as C
import math

import numpy as np

from oracle import pyoracle as po

F32 = np.float32
PI = F32(math.pi)                      # std.math.pi coerced to f32 (:73)
NUM_VALUES = (16, 4, 64, 16, 16, 16, 16, 2, 2, 8, 16, 4, 64, 16, 16, 16, 16, 2, 2, 2, 2, 2)       # :376-397
DEFAULT_PATCH = (2, 0, 0, 8, 8, 1, 8, 0, 0, 0, 1, 0, 0, 8, 8, 1, 8, 0, 0, 1, 1, 1)                # :376-397
(MOD_FREQ_MUL, MOD_WAVEFORM, MOD_VOLUME, MOD_ATTACK, MOD_DECAY, MOD_SUSTAIN, MOD_RELEASE, MOD_TREMOLO, MOD_VIBRATO, MOD_FEEDBACK,
 CAR_FREQ_MUL, CAR_WAVEFORM, CAR_VOLUME, CAR_ATTACK, CAR_DECAY, CAR_SUSTAIN, CAR_RELEASE, CAR_TREMOLO, CAR_VIBRATO,
 TREMOLO_DEPTH, VIBRATO_DEPTH, ALGORITHM) = range(22)
# musl sinf's argument classes by |x|: < pi/4, < 5pi/4, < 9pi/4, beyond (the thresholds as musl compares them, on the bits)
CLASS_BITS = (0x3f490fda, 0x407b53d1, 0x40e231d5)


def powf(x, y):
    return F32(po.lib().zo_math_powf(float(F32(x)), float(F32(y))))


def decibels(db):                                                    # :22-24
    return powf(10.0, F32(db) / F32(20))


def sinf(x):
    x = np.ascontiguousarray(x, F32)
    out = np.empty_like(x)
    po.lib().zo_math_sinf_n(po.fptr(x), po.fptr(out), x.size)
    return out


def _time(v):                                                        # :160
    return F32(0.002) + F32(4.0) * powf(F32(1) - F32(v) / F32(15.0), 3.0)


def _bits_db(value, table):
    db = F32(0)
    for bit, step in table:
        if value & bit:
            db = db - F32(step)
    return decibels(db)


def op_constants(freq_mul, volume, attack, decay, sustain, release, tremolo, vibrato, tremolo_depth, vibrato_depth):
    """Operator.paint :135-191 -> dict of np.float32"""
    fm = {0: 0.5, 11: 10.0, 12: 12.0, 13: 12.0, 14: 15.0, 15: 15.0}.get(freq_mul, float(freq_mul))
    return {
        "freq_mul": F32(fm),
        "volume": _bits_db(volume, ((32, 24.0), (16, 12.0), (8, 6.0), (4, 3.0), (2, 1.5), (1, 0.75))),
        "attack": _time(attack), "decay": _time(decay), "release": _time(release),
        "sustain": _bits_db(sustain, ((8, 24.0), (4, 12.0), (2, 6.0), (1, 3.0))),
        "tremolo": (F32(1) - decibels(-4.8 if tremolo_depth else -1.0)) if tremolo else F32(0),
        "vibrato": (powf(2.0, F32((14.0 if vibrato_depth else 7.0) / 1200.0)) - F32(1)) if vibrato else F32(0),
    }


FEEDBACK = tuple(F32(x) for x in (0.0, math.pi / 16, math.pi / 8, math.pi / 4, math.pi / 2, math.pi, math.pi * 2, math.pi * 4))   # :193-203


def patch_constants(patch):
    """one patch (22 values) -> (modulator constants, carrier constants, modulator feedback, waveforms (m, c), algorithm)"""
    p = [int(x) for x in patch]
    assert len(p) == 22 and all(0 <= v < n for v, n in zip(p, NUM_VALUES)), p
    td, vd = p[TREMOLO_DEPTH], p[VIBRATO_DEPTH]
    m = op_constants(p[MOD_FREQ_MUL], p[MOD_VOLUME], p[MOD_ATTACK], p[MOD_DECAY], p[MOD_SUSTAIN], p[MOD_RELEASE], p[MOD_TREMOLO], p[MOD_VIBRATO], td, vd)
    c = op_constants(p[CAR_FREQ_MUL], p[CAR_VOLUME], p[CAR_ATTACK], p[CAR_DECAY], p[CAR_SUSTAIN], p[CAR_RELEASE], p[CAR_TREMOLO], p[CAR_VIBRATO], td, vd)
    return m, c, FEEDBACK[p[MOD_FEEDBACK]], (p[MOD_WAVEFORM], p[CAR_WAVEFORM]), p[ALGORITHM]


def waveform(w, s, s2):
    """:75-80 as functions of s = sin(p) and s2 = sin(p * 2); `w` per voice"""
    a = np.abs(s)
    zero = np.zeros_like(s)
    out = np.where(w == 1, np.where(s > 0, s, zero), s)
    out = np.where(w == 2, a, out)
    return np.where(w == 3, np.where(s2 >= 0, a, zero), out).astype(F32)


STATE_DTYPE = np.dtype([("t", "<f4"), ("feedback1", "<f4"), ("feedback2", "<f4"), ("reserved", "<u4"),
                        ("env_state", "<u4"), ("env_t", "<f4"), ("env_last_value", "<f4"), ("env_start", "<f4")])


class FMRef:
    """n_voices Instruments; `group` consecutive voices share a patch and an LFO row."""

    def __init__(self, n_voices, group=1, patches=None):
        self.V, self.group = n_voices, group
        self.NI = -(-n_voices // group)
        L = po.lib()
        self.t = np.zeros((2, n_voices), F32)
        self.fb1 = np.zeros((2, n_voices), F32)
        self.fb2 = np.zeros((2, n_voices), F32)
        self.env = [(po.Envelope * max(n_voices, 1))(), (po.Envelope * max(n_voices, 1))()]
        for op in range(2):
            for v in range(n_voices):
                L.zo_envelope_init(C.byref(self.env[op][v]))
        self.classes = np.zeros((2, 4), np.int64)                    # [operator][|p| class]
        self.last_p, self.last_samples = [None, None], [None, None]
        self.stages = set()                                          # envelope states seen after a paint
        self.set_patches([DEFAULT_PATCH] if patches is None else patches)

    def set_patches(self, patches):
        patches = [list(p) for p in patches]
        if len(patches) == 1:
            patches = patches * self.NI
        assert len(patches) == self.NI
        self.patches = patches
        per = [patch_constants(p) for p in patches]
        idx = np.arange(self.V) // self.group
        self.k = [{name: np.array([per[j][op][name] for j in idx], F32) for name in per[0][0]} for op in range(2)] if self.V else [{}, {}]
        self.fb_amount = [np.array([per[j][2] for j in idx], F32), np.zeros(self.V, F32)]                 # the carrier's is 0 (:346)
        self.wave = [np.array([per[j][3][op] for j in idx], np.int32) for op in range(2)]
        self.alg = np.array([per[j][4] for j in idx], np.int32)

    # ---- state in the layout of zh_fm_state (two zh_fm_op_state)
    def state(self):
        st = np.zeros((self.V, 2), STATE_DTYPE)
        for op in range(2):
            st["t"][:, op], st["feedback1"][:, op], st["feedback2"][:, op] = self.t[op], self.fb1[op], self.fb2[op]
            for v in range(self.V):
                e = self.env[op][v]
                st[v, op]["env_state"], st[v, op]["env_t"] = e.state, e.painter.t
                st[v, op]["env_last_value"], st[v, op]["env_start"] = e.painter.last_value, e.painter.start
        return st

    def _envelope(self, op, voices, start, end, nic, sample_rate, note_on):
        """temps[1] = 0 + envelope (:229-237) -> [len(voices)][end - start]"""
        L = po.lib()
        out = np.zeros((len(voices), end), F32)
        k = self.k[op]
        for r, v in enumerate(voices):
            prm = po.EnvelopeParams(sample_rate, po.curve(po.CURVE_CUBED, k["attack"][v]), po.curve(po.CURVE_CUBED, k["decay"][v]),
                                    po.curve(po.CURVE_CUBED, k["release"][v]), float(k["sustain"][v]), 1 if note_on[r] else 0)
            L.zo_envelope_paint(C.byref(self.env[op][v]), start, end, po.fptr(out[r]), 1 if nic[r] else 0, C.byref(prm))
            self.stages.add(int(self.env[op][v].state))
        return out[:, start:end]

    def paint(self, start, end, nic, sample_rate, trem, vib, freq, note_on, voices=None):
        """Instrument.paint (:287-355) of `voices` (default: all) over [start, end).  nic / freq / note_on: per listed voice (or
        scalars); trem / vib: [n_instruments][frames].  Updates the state and returns (m, c, add_m): what the modulator and
        the carrier add to the output, [len(voices)][end - start], and which voices add m (algorithm 0)."""
        voices = np.arange(self.V) if voices is None else np.asarray(voices, np.int64)
        nv, n = len(voices), end - start
        bc = lambda x, dt: np.broadcast_to(np.asarray(x, dt), (nv,)).copy()
        nic, note_on, freq = bc(nic, bool), bc(note_on, bool), bc(freq, F32)
        sr = F32(sample_rate)
        inv_sr = F32(1.0) / sr                                       # :66
        inst = voices // self.group
        trem_in = np.ascontiguousarray(np.asarray(trem, F32)[inst, start:end])
        vib_in = np.ascontiguousarray(np.asarray(vib, F32)[inst, start:end])
        zero = F32(0)
        one = F32(1)
        alg1 = self.alg[voices] == 1
        outs = []
        phase = np.zeros((nv, n), F32)                               # modulator: phase = null -> 0 (:70)
        for op in range(2):
            k = {name: a[voices] for name, a in self.k[op].items()}
            fba, w = self.fb_amount[op][voices], self.wave[op][voices]
            # temps[1] = ((0 + vib_in * vibrato) + 1) * (freq * freq_mul)   :206-209
            f = ((zero + vib_in * k["vibrato"][:, None]) + one) * (freq * k["freq_mul"])[:, None]
            tr = (zero + trem_in * k["tremolo"][:, None]) + one      # :223-225
            e = self._envelope(op, voices, start, end, nic, float(sr), note_on)
            t, fb1, fb2 = self.t[op][voices].copy(), self.fb1[op][voices].copy(), self.fb2[op][voices].copy()
            samples, ps = np.zeros((nv, n), F32), np.zeros((nv, n), F32)
            any3 = bool((w == 3).any())
            for i in range(n):
                feedback = (fb1 + fb2) * fba                         # :71
                p = (t + phase[:, i]) * PI * F32(2) + feedback       # :73
                s = sinf(p)
                s2 = sinf(p * F32(2)) if any3 else s
                sample = waveform(w, s, s2)
                samples[:, i], ps[:, i] = sample, p
                t = t + f[:, i] * inv_sr                             # :84
                fb2 = fb1
                fb1 = sample
                pb = np.abs(p).view(np.uint32)
                cls = (pb > CLASS_BITS[0]).astype(int) + (pb > CLASS_BITS[1]) + (pb > CLASS_BITS[2])
                self.classes[op] += np.bincount(cls, minlength=4)
            self.t[op][voices] = t - np.trunc(t)                     # :64
            self.last_p[op], self.last_samples[op] = ps, samples     # of the last paint() call, for the tests of this helper
            self.fb1[op][voices], self.fb2[op][voices] = fb1, fb2
            o = ((zero + samples) * k["volume"][:, None]) * tr       # temps[0] :212-226
            out = o * e                                              # multiply :240 (added to the output, or to a zeroed temp)
            outs.append(out.astype(F32))
            if op == 0:
                # algorithm 1: the modulator went into a zeroed temp that is the carrier's phase (:305-310)
                phase = np.where(alg1[:, None], zero + out, zero).astype(F32)
        return outs[0], outs[1], ~alg1

    def paint_into(self, out, start, end, nic, sample_rate, trem, vib, freq, note_on, voices=None):
        """paint() added into out [n_voices][frames] as the reference does: (out + m) + c, or out + c (algorithm 1)"""
        voices = np.arange(self.V) if voices is None else np.asarray(voices, np.int64)
        m, c, add_m = self.paint(start, end, nic, sample_rate, trem, vib, freq, note_on, voices)
        add_into(out, voices, start, end, m, c, add_m)

    def paint_spans(self, start, end, sample_rate, trem, vib, table):
        """The Trigger loop (:457-496) for every voice: table = {count [V], start / end / freq / note_on / note_id_changed [K][V]}
        with well-formed lists (ascending, inside [start, end)).  -> (m, c [V][frames], painted [V][frames] bool, add_m [V])"""
        F = np.asarray(trem).shape[1]
        m, c = np.zeros((self.V, F), F32), np.zeros((self.V, F), F32)
        painted = np.zeros((self.V, F), bool)
        K = int(np.max(table["count"])) if self.V else 0
        prev_end = np.full(self.V, start, np.int64)
        for k in range(K):
            groups = {}
            for v in np.nonzero(table["count"] > k)[0]:
                groups.setdefault((int(table["start"][k, v]), int(table["end"][k, v])), []).append(int(v))
            for (s, e), vs in groups.items():
                vs = np.array(vs)
                assert (prev_end[vs] <= s).all() and s <= e <= end, "the helper takes well-formed tables only"
                prev_end[vs] = e
                mm, cc, _ = self.paint(s, e, table["note_id_changed"][k, vs] != 0, sample_rate, trem, vib, table["freq"][k, vs],
                                       table["note_on"][k, vs] != 0, vs)
                m[vs, s:e], c[vs, s:e], painted[vs, s:e] = mm, cc, True
        return m, c, painted, self.alg == 0


def add_into(out, voices, start, end, m, c, add_m):
    o = out[voices, start:end]
    o1 = np.where(add_m[:, None], o + m, o)
    out[voices, start:end] = (o1 + c).astype(F32)


def add_spans_into(out, m, c, painted, add_m):
    """a span paint onto out [V][F]"""
    o1 = np.where(add_m[:, None], out + m, out)
    return np.where(painted, o1 + c, out).astype(F32)


def split_image(base, m, c, painted, add_m):
    """ZH_FM_SPLIT_OPERATORS onto base [2V][F]: row 2v += m (algorithm 0), row 2v + 1 += c"""
    out = base.copy()
    out[0::2] = np.where(painted & add_m[:, None], base[0::2] + m, base[0::2])
    out[1::2] = np.where(painted, base[1::2] + c, base[1::2])
    return out.astype(F32)


def mix_voices(m, c, painted, add_m, polyphony):
    """what MainModule's voices add into ONE zeroed buffer per synth, in voice order (:457-496): (acc + m_v) + c_v, or acc + c_v
    -> [n_synths][frames]"""
    V, F = m.shape
    acc = np.zeros((V // polyphony, F), F32)
    for j in range(V // polyphony):
        for i in range(polyphony):
            v = j * polyphony + i
            a1 = (acc[j] + m[v]) if add_m[v] else acc[j]
            acc[j] = np.where(painted[v], a1 + c[v], acc[j])
    return acc


# ---- MainModule (:358-497) for N synths
class NoteParams(C.Structure):                                       # :365-368
    _fields_ = [("freq", C.c_float), ("note_on", C.c_uint8), ("pad", C.c_uint8 * 3)]


REC = np.dtype([("freq", "<f4"), ("on", "u1"), ("pad", "u1", 3)])
ON_OFFSET = 4
LFO_TREMOLO_HZ, LFO_VIBRATO_HZ = 3.7, 6.4                            # :437-450


class MainModuleRef:
    """N independent MainModules: per synth an ImpulseQueue, a PolyphonyDispatcher(polyphony) and a Trigger per voice (the
    host classes of zang_amd/notes.py), the two LFOs from the oracle's SineOsc, and the voices from FMRef."""

    def __init__(self, n_synths, patches=None, polyphony=8, sample_rate=48000.0):
        from zang_amd import notes
        self.N, self.P, self.sr = n_synths, polyphony, float(sample_rate)
        ns = notes.Notes(NoteParams)
        self.iq = [ns.ImpulseQueue() for _ in range(n_synths)]
        self.dispatcher = [ns.PolyphonyDispatcher(polyphony)() for _ in range(n_synths)]
        self.trigger = [[notes.Trigger(NoteParams)() for _ in range(polyphony)] for _ in range(n_synths)]
        self.fm = FMRef(n_synths * polyphony, polyphony, patches)
        L = po.lib()
        self.lfo = [(po.SineOsc(), po.SineOsc()) for _ in range(n_synths)]
        for a, b in self.lfo:
            L.zo_sineosc_init(C.byref(a)); L.zo_sineosc_init(C.byref(b))
        self.max_spans = 0

    def push(self, synth, frame, note_id, freq, note_on):
        self.iq[synth].push(int(frame), int(note_id), NoteParams(float(freq), 1 if note_on else 0))

    def lfos(self, frames):
        L = po.lib()
        trem, vib = np.zeros((self.N, frames), F32), np.zeros((self.N, frames), F32)
        for j, (a, b) in enumerate(self.lfo):
            L.zo_sineosc_paint(C.byref(a), 0, frames, po.fptr(trem[j]), self.sr, po.constant(LFO_TREMOLO_HZ), po.constant(0.0))
            L.zo_sineosc_paint(C.byref(b), 0, frames, po.fptr(vib[j]), self.sr, po.constant(LFO_VIBRATO_HZ), po.constant(0.0))
        return trem, vib

    def table(self, frames):
        """this buffer's Trigger sub-spans of every voice, as a span table"""
        from zang_amd.zang import Span
        V = self.N * self.P
        per = [[] for _ in range(V)]
        for j in range(self.N):
            poly = self.dispatcher[j].dispatch(self.iq[j].consume())
            for i in range(self.P):
                tr = self.trigger[j][i]
                ctr = tr.counter(Span(0, frames), poly[i])
                while True:
                    r = tr.next(ctr)
                    if r is None:
                        break
                    per[j * self.P + i].append((r.span.start, r.span.end, r.params.freq, r.params.note_on != 0, r.note_id_changed))
        K = max([len(s) for s in per] + [1])
        self.max_spans = max(self.max_spans, K)
        tb = {"count": np.array([len(s) for s in per], np.uint32), "start": np.zeros((K, V), np.uint32), "end": np.zeros((K, V), np.uint32),
              "freq": np.zeros((K, V), F32), "note_on": np.zeros((K, V), np.uint8), "note_id_changed": np.zeros((K, V), np.uint8)}
        for v, spans in enumerate(per):
            for k, (s, e, f, on, nic) in enumerate(spans):
                tb["start"][k, v], tb["end"][k, v], tb["freq"][k, v], tb["note_on"][k, v], tb["note_id_changed"][k, v] = s, e, f, on, nic
        return tb

    def paint(self, frames):
        """MainModule.paint over a zeroed output -> [n_synths][frames]"""
        trem, vib = self.lfos(frames)
        tb = self.table(frames)
        m, c, painted, add_m = self.fm.paint_spans(0, frames, self.sr, trem, vib, tb)
        return mix_voices(m, c, painted, add_m, self.P)
