"""The hostile-parameter table: every float parameter slot and carried state word of a module with a non-finite, zero, negative,
denormal, huge or threshold value in it, ONE slot of the module's ordinary tuple at a time (plus a few pairs of slots that
interact), laid out so that a hostile voice meets the wave and workgroup votes of the kernels both alone among ordinary
neighbours and among hostile voices only.  Not a test module: tests/test_cpp_hostile_oracle.py runs the table through the oracle
under the sanitizers (tests/cpp/hostile_oracle.c) and asserts that it is worth comparing against; tests/test_gpu_hostile_params.py
paints it on the device in every kernel form and compares with the oracle.

A voice is a `Rec`: eight float parameters `p` (the module's slots first), a note script `k`, optional carried state words `st`,
and its own columns of the images a module reads (`cin` the input, `cctl` / `cc2` the control images) and of the garbage the
output image holds before the first paint.  What a whole paint shares -- the sample rate, a filter type, curve tags, which slots
come from an image -- is a `Variant`; a module is painted once per variant and chunk.

The script (SPANS): 352 rows; span (13, 334) with ZERO_FIRST over the garbage, then (0, 352), an empty span and (200, 334), all
three adding, state carried.  Envelope and Portamento get one of NOTES per voice: (note_id_changed, note_on) of every paint.

Layout of a chunk of V = 1,024 voices in groups of G (64: a wave; 256: the voices of a four-voices-per-lane workgroup):
G = 64: wave 0 ordinary throughout, waves 1..14 one hostile voice each among 63 ordinary ones, wave 15 hostile voices only;
G = 256: groups 0..2 one hostile voice each among 255 ordinary ones (three of such a group's four waves are ordinary
throughout), group 3 hostile voices only.  The hostile-only group cycles through the variant's hostile voices, starting further
on in every chunk.  The sample rate is one value per paint: a hostile sample rate is a variant of its own, painted over a chunk of
ordinary voices with a few hostile frequencies (the freq x sample_rate pairs) in wave 1 and compared at SR_CHECK sampled voices.
"""
import copy
import ctypes as C
import struct

import numpy as np

F = 352
SPANS = [(13, 334), (0, 352), (120, 120), (200, 334)]
SR = 48000.0
V = 1024
NP = 8                     # floats of Rec.p
NST = 12                   # state words
MAIN_DELAY = 400           # StereoEchoes' main delay (its halves: 200): the least lengths its role-wave form takes are 385 / 192
NEX = 352 + 2 * MAIN_DELAY # floats of further state a record's result carries (a delay ring; StereoEchoes: the right output and three rings)
DELAY = 192                # delay samples of the echoes: the least the role-wave form takes
MAGIC = 0x534F485A         # "ZHOS"

f32 = np.float32
_H = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 1e-30, 3e38, -3e38, -1.0, 1.0, 2.0, 1e9, 4.3e9]
HOSTILE = [f32(x) for x in _H]


def around(x):
    """the f32 threshold x and one ulp either side of it"""
    x = f32(x)
    return [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]


def bits(x):
    return int(np.asarray(x, f32).view(np.uint32))


def with_thresholds(*thr):
    """the hostile list plus every threshold's three values, no bit pattern twice"""
    out, seen = [], set()
    for x in HOSTILE + [y for t in thr for y in around(t)]:
        if bits(x) not in seen:
            seen.add(bits(x)); out.append(f32(x))
    return out


# (note_id_changed, note_on) of the four paints: held; released inside the empty span; retriggered twice; late; never on
NOTES = [[(1, 1), (0, 1), (0, 1), (0, 1)],
         [(1, 1), (0, 1), (1, 0), (0, 0)],
         [(1, 1), (1, 1), (0, 1), (1, 1)],
         [(0, 0), (0, 0), (1, 1), (0, 1)],
         [(0, 0), (0, 0), (0, 0), (0, 0)]]
IMG_ROWS = np.r_[20:120, 250:260]         # the rows of a control / input image that hold a record's hostile value
SR_CHECK = 40                             # voices compared in a hostile-sample-rate variant

SINE, PULSE, TRISAW, CYCLE, ENVELOPE, PORTAMENTO, DECIMATOR, DISTORTION, FILTER, NICE, PMOSC, ECHOES, CURVE, GATE, SAMPLER, NOISEFILTER, FSAW, HSQUARE, STEREO = range(19)


class Variant:
    def __init__(self, sr=SR, vi=(), label="", whole_paint=False):
        self.sr = f32(sr)
        self.vi = tuple(vi) + (0,) * (6 - len(vi))
        self.label = label or "default"
        # what is hostile is shared by every voice of the paint (the sample rate; a Curve's nodes): one chunk, sampled voices compared
        self.shared_by_paint = whole_paint or bits(self.sr) != bits(SR)

    def key(self):
        return (bits(self.sr), self.vi)

    def __repr__(self):
        return f"sr={self.sr!r} {self.label}"


class Rec:
    __slots__ = ("p", "k", "st", "cin", "cctl", "cc2", "garbage", "hostile", "base", "label", "ref", "ref_st", "ref_ex", "ref_batch", "slot")

    def __init__(self, p, seed, k=0, st=None, hostile=False, base=None, label="", slot=""):
        self.p = np.zeros(NP, f32); self.p[:len(p)] = p
        self.k, self.st, self.hostile, self.base, self.label, self.slot = k, st, hostile, base, label, slot
        g = np.random.default_rng(90000 + seed)
        self.garbage = g.uniform(-2, 2, F).astype(f32)
        self.cin = g.uniform(-1, 1, F).astype(f32)
        self.cctl = (1.0 + 0.25 * g.random(F)).astype(f32)      # (the module scales or replaces it: Module.columns)
        self.cc2 = g.uniform(0.0, 0.9, F).astype(f32)
        self.ref = self.ref_st = self.ref_ex = self.ref_batch = None


def _ordinary_params():
    from zang_amd import workloads
    return workloads.voice_params(5, 0, V)


class Module:
    """One module's slots, ordinary tuple, variants and hostile records.  Subclasses: `mid`, `name`, `slots`, `group`,
    `state` (names of the device's state fields, in the order of Rec.st / the oracle harness's state words; "u:" marks an
    integer word), ordinary(v), variants(), hostile(variant)."""
    group = 64
    state = ()

    def __init__(self):
        self.freq, self.color, self.u2, self.u3 = _ordinary_params()
        self._ord = {}
        self._host = {}

    # ---- records
    def columns(self, r, variant):
        """fit a fresh record's control columns to the module (an oscillator's frequency image wobbles around p[0])"""

    def rec(self, variant, v, seed=None, repl=None, img=None, whole=None, **kw):
        """the ordinary tuple of voice v with the slots of `repl` {slot: value} replaced, the rows IMG_ROWS of the columns of
        `img` {column: value} set, and the columns of `whole` {column: value} filled"""
        p = np.array(self.ordinary(v), f32)
        for s, x in (repl or {}).items():
            p[self.slots.index(s)] = x
        r = Rec(p, v if seed is None else seed, **kw)
        self.columns(r, variant)
        for c, x in (img or {}).items():
            getattr(r, c)[IMG_ROWS] = x
        for c, x in (whole or {}).items():
            getattr(r, c)[:] = x
        return r

    def ordinary_rec(self, variant, v):
        key = (variant.key(), v)
        if key not in self._ord:
            if variant.shared_by_paint:                     # the same voice at another sample rate: the columns are shared
                r = copy.copy(self._plain_rec(variant, v))
                r.ref = r.ref_st = r.ref_ex = r.ref_batch = None
                self._ord[key] = r
            else:
                self._ord[key] = self.rec(variant, v, k=v % 3 if v % 11 else 3, label=f"ordinary {v}")
        return self._ord[key]

    def _plain_rec(self, variant, v):
        """the voice's record under the same variant at the ordinary sample rate: its columns are shared"""
        return self.ordinary_rec(Variant(SR, variant.vi), v)

    def hostile_recs(self, variant):
        """the variant's hostile records, each with its ordinary counterpart as .base"""
        key = variant.key()
        if key not in self._host:
            out = []
            for i, spec in enumerate(self.hostile(variant)):
                v = (17 * i + 3) % 64
                k = spec.pop("k", i % 3)
                label = spec.pop("label")
                base = self.rec(variant, v, seed=2000 + i, k=k, label="base of " + label)
                out.append(self.rec(variant, v, seed=2000 + i, k=k, hostile=True, base=base, label=label, **spec))
            self._host[key] = out
        return self._host[key]

    def slot_specs(self, variant, slot, values, image=None):
        """one record per value in `slot`: in the parameter, or in the rows IMG_ROWS of column `image`"""
        for x in values:
            if image:
                yield dict(img={image: x}, label=f"{slot} image={x!r}", slot=slot)
            else:
                yield dict(repl={slot: x}, label=f"{slot}={x!r}", slot=slot)

    def state_specs(self, word_sets, prefix="state"):
        for st in word_sets:
            yield dict(st=list(st), label=f"{prefix} {st!r}", slot="state")

    # ---- chunks
    def chunks(self, variant, n_voices=V):
        """The variant's chunks, each a list of n_voices records in voice order (the layout of the module's docstring): as many
        chunks as it takes for every hostile record to stand alone in a group once.  A hostile sample rate: one chunk."""
        G = self.group
        if variant.shared_by_paint:
            recs = [self.ordinary_rec(variant, v) for v in range(V)]
            for j, r in enumerate(self.hostile_recs(variant)):
                recs[64 + 7 * j + 1] = r
            return [recs[:n_voices]]
        host = self.hostile_recs(variant)
        n_groups = V // G
        alone = n_groups - 2 if G == 64 else n_groups - 1
        first = 1 if G == 64 else 0
        out = []
        for c in range((len(host) + alone - 1) // alone):
            recs = [self.ordinary_rec(variant, v) for v in range(V)]
            for j, r in enumerate(host[c * alone:(c + 1) * alone]):
                recs[(first + j) * G + (37 * (c * alone + j) + 5) % G] = r
            for j in range(G):
                recs[(n_groups - 1) * G + j] = host[(c * G + j) % len(host)]
            out.append(recs[:n_voices])
        return out

    def checked(self, variant, recs):
        """indices of the voices of a chunk that are compared"""
        if not variant.shared_by_paint:
            return np.arange(len(recs))
        idx = set(range(0, len(recs), max(1, len(recs) // SR_CHECK))) | {len(recs) - 1}
        idx |= {i for i, r in enumerate(recs) if r.hostile}
        return np.array(sorted(idx))

    def sr_variants(self, vi=(), label=""):
        return [Variant(x, vi, f"{label} hostile sample rate".strip()) for x in HOSTILE]

    def all_hostile(self):
        """[(variant, record)]: every hostile record once, and SR_CHECK-many voices of every hostile-sample-rate variant"""
        out = []
        for va in self.variants():
            out += [(va, r) for r in self.hostile_recs(va)]
            if va.shared_by_paint:
                out += [(va, self.ordinary_rec(va, v)) for v in range(0, V, V // 8)]
        return out


def _freq_pairs(slot="freq"):
    return [dict(repl={slot: x}, label=f"{slot}={x!r} x sample rate", slot=slot) for x in (f32(np.nan), f32(0.0), f32(np.inf), f32(-1.0), f32(1e9))]


class SineOsc(Module):
    mid, name, slots, state = SINE, "SineOsc", ("freq", "phase"), ("t",)

    def ordinary(self, v):
        return [self.freq[v], 0.25 * self.u2[v]]

    def columns(self, r, variant):
        with np.errstate(over="ignore", invalid="ignore"):
            r.cctl *= r.p[0]

    def variants(self):
        return [Variant(vi=(0, 0), label="constant"), Variant(vi=(1, 1), label="freq and phase images")] + self.sr_variants() + \
               [Variant(x, (1, 0), "freq image, hostile sample rate") for x in HOSTILE[:5]]

    def hostile(self, va):
        if va.shared_by_paint:
            yield from _freq_pairs()
            return
        fi, pi = va.vi[0], va.vi[1]
        yield from self.slot_specs(va, "freq", with_thresholds(SR / 8), "cctl" if fi else None)
        yield from self.slot_specs(va, "phase", HOSTILE, "cin" if pi else None)
        for fq, ph in ((0.0, 0.0), (-0.0, -0.0), (0.0, 1.0), (np.inf, np.nan), (1e9, 1e9)):                              # freq x phase
            yield dict(repl={"freq": f32(fq), "phase": f32(ph)}, label=f"freq={fq!r} x phase={ph!r}", slot="pair")
        yield from self.state_specs([[f32(x)] for x in (1e9, 3e38, np.nan, np.inf, -1e9, 16777216.0)], "t")


class _PhaseOsc(Module):
    slots, group = ("freq", "color"), 256

    def ordinary(self, v):
        return [self.freq[v], self.color[v]]

    def columns(self, r, variant):
        with np.errstate(over="ignore", invalid="ignore"):
            r.cctl *= r.p[0]

    def variants(self):
        return [Variant(vi=(0,), label="constant"), Variant(vi=(1,), label="freq image")] + self.sr_variants() + \
               [Variant(x, (1,), "freq image, hostile sample rate") for x in HOSTILE[:5]]

    def hostile(self, va):
        if va.shared_by_paint:
            yield from _freq_pairs()
            return
        yield from self.slot_specs(va, "freq", with_thresholds(SR / 8, 0.0), "cctl" if va.vi[0] else None)
        yield from self.slot_specs(va, "color", with_thresholds(0.0, 1.0))
        # cnt within two ifreq of 2^32 (ifreq of the record's own ordinary frequency is below 2^29: sr/8)
        for d in (1, 1 << 20, 1 << 27, 1 << 29):
            yield dict(st=self.state_words((1 << 32) - d), label=f"cnt=2^32-{d}", slot="state")
        yield from self.more_states()

    def more_states(self):
        return ()


class PulseOsc(_PhaseOsc):
    mid, name, state = PULSE, "PulseOsc", ("u:cnt",)

    def state_words(self, cnt):
        return [int(cnt)]


class TriSawOsc(_PhaseOsc):
    mid, name, state = TRISAW, "TriSawOsc", ("u:cnt", "t")

    def state_words(self, cnt):
        return [int(cnt), f32(0.0)]

    def more_states(self):
        for x in (1e9, 3e38, np.nan, np.inf):
            yield dict(st=[0, f32(x)], label=f"t={x!r}", slot="state")


class Cycle(Module):
    mid, name, slots, state = CYCLE, "Cycle", ("speed",), ("t",)

    def ordinary(self, v):
        return [self.freq[v]]

    def columns(self, r, variant):
        with np.errstate(over="ignore", invalid="ignore"):
            r.cctl *= r.p[0]

    def variants(self):
        return [Variant(vi=(0,), label="constant"), Variant(vi=(1,), label="speed image")] + self.sr_variants()

    def hostile(self, va):
        if va.shared_by_paint:
            yield from _freq_pairs("speed")
            return
        yield from self.slot_specs(va, "speed", with_thresholds(SR), "cctl" if va.vi[0] else None)
        yield from self.state_specs([[f32(x)] for x in (1e9, 3e38, np.nan, np.inf, -0.5, 1.0)], "t")


_PAINTER = [f32(x) for x in (np.nan, 1.5, -0.5, np.inf, -np.inf)]
_TAGS = ["instantaneous", "linear", "squared", "cubed"]


class Envelope(Module):
    mid, name, slots = ENVELOPE, "Envelope", ("attack", "decay", "release", "sustain_volume")
    state = ("u:state", "t", "last_value", "start")

    def ordinary(self, v):
        return [0.0005 + 0.003 * self.u2[v], 0.001 + 0.003 * self.u3[v], 0.001 + 0.004 * self.u2[v], 0.2 + 0.6 * self.u3[v]]

    def variants(self):
        return [Variant(vi=(t, t, t), label=_TAGS[t]) for t in range(4)] + [Variant(vi=(1, 3, 2), label="linear / cubed / squared")] + \
               self.sr_variants((3, 3, 3), "cubed,")

    def hostile(self, va):
        if va.shared_by_paint:
            yield from [dict(repl={"attack": x}, label=f"attack={x!r} x sample rate", slot="attack") for x in (f32(np.nan), f32(0.0), f32(1e9))]
            return
        for s in self.slots[:3]:
            yield from self.slot_specs(va, s, HOSTILE)
        yield from self.slot_specs(va, "sustain_volume", with_thresholds(0.0, 1.0))
        for a, s in ((0.0, np.nan), (np.nan, 2.0), (np.inf, 0.0), (-1.0, -1.0), (1e-45, 1.0), (3e38, np.inf)):      # attack x sustain
            yield dict(repl={"attack": f32(a), "sustain_volume": f32(s)}, label=f"attack={a!r} x sustain={s!r}", slot="pair")
        for i, x in enumerate(_PAINTER):
            yield dict(st=[1 + i % 4, x, f32(0.3), f32(0.1)], label=f"painter t={x!r}", slot="state", k=3 if i % 2 else 0)
            yield dict(st=[1 + (i + 1) % 4, f32(0.4), x, f32(0.1)], label=f"painter last_value={x!r}", slot="state", k=3 if i % 2 else 1)
            yield dict(st=[1 + (i + 2) % 4, f32(0.4), f32(0.3), x], label=f"painter start={x!r}", slot="state", k=3 if i % 2 else 2)


class Portamento(Module):
    mid, name, slots, state = PORTAMENTO, "Portamento", ("duration", "goal"), ("t", "last_value", "start")

    def ordinary(self, v):
        return [0.0005 + 0.006 * self.u2[v], self.freq[v]]

    def variants(self):
        return [Variant(vi=(t,), label=_TAGS[t]) for t in range(4)] + self.sr_variants((3,), "cubed,")

    def hostile(self, va):
        if va.shared_by_paint:
            yield from [dict(repl={"duration": x}, label=f"duration={x!r} x sample rate", slot="duration") for x in (f32(np.nan), f32(0.0), f32(1e9))]
            return
        yield from self.slot_specs(va, "duration", HOSTILE)
        yield from self.slot_specs(va, "goal", HOSTILE)
        for i, x in enumerate(_PAINTER):
            yield dict(st=[x, f32(300.0), f32(100.0)], label=f"painter t={x!r}", slot="state", k=3 if i % 2 else 0)
            yield dict(st=[f32(0.4), x, f32(100.0)], label=f"painter last_value={x!r}", slot="state", k=3 if i % 2 else 1)
            yield dict(st=[f32(0.4), f32(300.0), x], label=f"painter start={x!r}", slot="state", k=3 if i % 2 else 2)


class Decimator(Module):
    mid, name, slots, state = DECIMATOR, "Decimator", ("fake_sample_rate",), ("dval", "dcount")

    def ordinary(self, v):
        return [self.freq[v] * f32(8.0)]

    def variants(self):
        return [Variant()] + self.sr_variants()

    def hostile(self, va):
        if va.shared_by_paint:
            yield from _freq_pairs("fake_sample_rate")
            return
        yield from self.slot_specs(va, "fake_sample_rate", with_thresholds(SR))
        yield from self.slot_specs(va, "input", HOSTILE, "cin")
        yield from self.state_specs([[f32(0.5), f32(x)] for x in (5.0, -3.0, 1.0, 1e6, np.nan, np.inf, -np.inf, 1e-45, -0.0, 0.99999994)], "dval, dcount")
        yield from self.state_specs([[f32(x), f32(0.25)] for x in (np.nan, np.inf, -0.0)], "dval, dcount")


class Distortion(Module):
    mid, name, slots, group = DISTORTION, "Distortion", ("ingain", "outgain", "offset"), 256

    def ordinary(self, v):
        return [0.1 + 0.85 * self.u2[v], 0.2 + 0.7 * self.u3[v], 0.4 * self.color[v] - 0.2]

    def variants(self):
        return [Variant(vi=(0,), label="overdrive"), Variant(vi=(1,), label="clip")]

    def hostile(self, va):
        for s in self.slots:
            yield from self.slot_specs(va, s, with_thresholds(0.0, 1.0) if s == "ingain" else HOSTILE)
        yield from self.slot_specs(va, "input", HOSTILE, "cin")
        for g, o in ((np.nan, np.inf), (0.0, np.nan), (np.inf, -np.inf), (1.0, 3e38), (3e38, 3e38), (1e-45, -1.0)):     # ingain x offset
            yield dict(repl={"ingain": f32(g), "offset": f32(o)}, label=f"ingain={g!r} x offset={o!r}", slot="pair")


_FILTER_STATES = [np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1e-45, -0.0, 0.0, 1e30, -1e25]
_FILTER_TYPES = ["bypass", "low_pass", "band_pass", "high_pass", "notch", "all_pass"]


class Filter(Module):
    mid, name, slots, state = FILTER, "Filter", ("cutoff", "res"), ("l", "b")

    def ordinary(self, v):
        return [self.color[v], 0.9 * self.u3[v]]

    def columns(self, r, variant):
        r.cctl[:] = (r.cctl - f32(1.0)) * f32(3.6) + f32(0.02)              # cutoffs in [0.02, 0.92)

    def variants(self):
        return [Variant(vi=(t, i, i), label=_FILTER_TYPES[t] + (", cutoff and resonance images" if i else ", constant")) for t in range(6) for i in (0, 1)]

    def hostile(self, va):
        i = va.vi[1]
        yield from self.slot_specs(va, "cutoff", with_thresholds(0.0, 1.0), "cctl" if i else None)
        yield from self.slot_specs(va, "res", with_thresholds(0.0, 1.0), "cc2" if i else None)
        yield from self.slot_specs(va, "input", HOSTILE, "cin")
        for j, x in enumerate(_FILTER_STATES):
            yield dict(st=[f32(x), f32(0.1)], label=f"l={x!r}", slot="state")
            yield dict(st=[f32(-0.2), f32(x)], label=f"b={x!r}", slot="state")


def _env_states(words):
    """painter words hostile one at a time inside a composite's state: words(state, t, last_value, start) -> the full state"""
    for i, x in enumerate(_PAINTER):
        yield dict(st=words(1 + i % 4, x, f32(0.3), f32(0.1)), label=f"env t={x!r}", slot="state", k=3 if i % 2 else 0)
        yield dict(st=words(1 + (i + 1) % 4, f32(0.4), x, f32(0.1)), label=f"env last_value={x!r}", slot="state", k=3 if i % 2 else 1)
        yield dict(st=words(1 + (i + 2) % 4, f32(0.4), f32(0.3), x), label=f"env start={x!r}", slot="state", k=3 if i % 2 else 2)


class NiceInstrument(Module):
    """PulseOsc -> Filter (cutoff from the frequency) times a cubed Envelope; `color` is the instrument's own"""
    mid, name, slots = NICE, "NiceInstrument", ("freq", "color")
    state = ("u:osc.cnt", "flt.l", "flt.b", "u:env.state", "env.t", "env.last_value", "env.start")

    def ordinary(self, v):
        return [self.freq[v], self.color[v]]

    def variants(self):
        return [Variant()] + self.sr_variants()

    def hostile(self, va):
        if va.shared_by_paint:
            yield from _freq_pairs()
            return
        yield from self.slot_specs(va, "freq", with_thresholds(SR / 8, SR / 64, 0.0))
        yield from self.slot_specs(va, "color", with_thresholds(0.0, 1.0))
        for d in (1, 1 << 20, 1 << 27, 1 << 29):
            yield dict(st=[(1 << 32) - d, f32(0), f32(0), 0, f32(0), f32(0), f32(0)], label=f"cnt=2^32-{d}", slot="state")
        for x in _FILTER_STATES:
            yield dict(st=[0, f32(x), f32(0.1), 0, f32(0), f32(0), f32(0)], label=f"l={x!r}", slot="state")
            yield dict(st=[0, f32(-0.2), f32(x), 0, f32(0), f32(0), f32(0)], label=f"b={x!r}", slot="state")
        yield from _env_states(lambda s, t, lv, st: [0, f32(0), f32(0), s, t, lv, st])


class PMOscInstrument(Module):
    """two SineOscs (the modulator into the carrier's phase) times a cubed Envelope; `release_duration` is the instrument's own"""
    mid, name, slots = PMOSC, "PMOscInstrument", ("freq", "release_duration")
    state = ("carrier.t", "modulator.t", "u:env.state", "env.t", "env.last_value", "env.start")

    def ordinary(self, v):
        return [self.freq[v], 0.001 + 0.004 * self.u2[v]]

    def variants(self):
        return [Variant()] + self.sr_variants()

    def hostile(self, va):
        if va.shared_by_paint:
            yield from _freq_pairs()
            return
        yield from self.slot_specs(va, "freq", with_thresholds(SR / 8, 0.0))
        yield from self.slot_specs(va, "release_duration", HOSTILE, )
        for x in (1e9, 3e38, np.nan, np.inf, -1e9):
            yield dict(st=[f32(x), f32(0.25), 0, f32(0), f32(0), f32(0)], label=f"carrier t={x!r}", slot="state")
            yield dict(st=[f32(0.25), f32(x), 0, f32(0), f32(0), f32(0)], label=f"modulator t={x!r}", slot="state")
        yield from _env_states(lambda s, t, lv, st: [f32(0.1), f32(0.2), s, t, lv, st])


class FilteredEchoes(Module):
    """a Delay of DELAY samples fed back through a low-pass Filter; the ring is compared as further state"""
    mid, name, slots, state = ECHOES, "FilteredEchoes", ("feedback_volume", "cutoff"), ("u:index", "l", "b")

    def ordinary(self, v):
        return [0.1 + 0.8 * self.u2[v], 0.05 + 0.9 * self.u3[v]]

    def variants(self):
        return [Variant()]

    def hostile(self, va):
        yield from self.slot_specs(va, "feedback_volume", with_thresholds(0.0, 1.0))
        yield from self.slot_specs(va, "cutoff", with_thresholds(0.0, 1.0))
        yield from self.slot_specs(va, "input", HOSTILE, "cin")
        for x in (0.0, -0.0):                                    # silence in: what is left is the filter's own dc offset
            yield dict(whole={"cin": f32(x)}, label=f"input all {x!r}", slot="input")
            yield dict(whole={"cin": f32(x)}, repl={"cutoff": f32(x)}, label=f"input all {x!r} x cutoff={x!r}", slot="pair")


def _curve_sets():
    """[(label, [(value, t)])]: the node lists of the Curve module's variants -- one list per paint, shared by every voice"""
    base = [(0.0, 0.0), (0.8, 0.0015), (-0.5, 0.003), (0.25, 0.0045), (1.0, 0.007), (-1.0, 0.009), (0.5, 0.012), (0.0, 0.015)]
    sets = [("ordinary", base)]
    for x in HOSTILE:
        sets.append((f"node 3 t={x!r}", base[:3] + [(0.25, x)] + base[4:]))
        sets.append((f"node 3 value={x!r}", base[:3] + [(x, 0.0045)] + base[4:]))
    sets += [("equal t", base[:2] + [(-0.5, 0.0015), (0.25, 0.0015)] + base[4:]), ("decreasing t", base[::-1]),
             ("negative t", [(v, t - 0.004) for v, t in base]), ("huge t", [(v, t * 1e12) for v, t in base]),
             ("every t NaN", [(v, np.nan) for v, t in base]), ("first t NaN", [(0.3, np.nan)] + base[1:]),
             ("last t -inf", base[:-1] + [(0.3, -np.inf)]), ("all values 0", [(0.0, t) for v, t in base]),
             ("all values -0", [(-0.0, t) for v, t in base]), ("one node", [(0.7, 0.002)]), ("one node at 0", [(0.7, 0.0)]),
             ("one node, t NaN", [(0.7, np.nan)]), ("no nodes", [])]
    return sets


CURVE_SETS = _curve_sets()


class Curve(Module):
    """The nodes are ONE list per paint: every variant is a node list (and a function) painted over a chunk of voices that differ in
    their note scripts; the list rides in the record's `cin` column as (value, t) pairs, its length in p[0]."""
    mid, name, slots = CURVE, "Curve", ()
    state = ("t", "u:current_song_note", "u:current_song_note_offset", "u:next_song_note")

    def ordinary(self, v):
        return [0.0]

    def columns(self, r, variant):
        nodes = CURVE_SETS[variant.vi[1]][1]
        r.p[0] = len(nodes)
        r.cin[:] = 0.0
        r.cin[:2 * len(nodes)] = np.array(nodes, f32).reshape(-1)

    def variants(self):
        return [Variant(SR, (fn, i), f"{('linear', 'smoothstep')[fn]}, {label}", whole_paint=True) for fn in (0, 1) for i, (label, _) in enumerate(CURVE_SETS)]

    def _plain_rec(self, variant, v):
        key = ("plain", variant.vi, v)
        if key not in self._ord:
            self._ord[key] = self.rec(variant, v, k=v % 4, label=f"voice {v}, {variant.label}")
        return self._ord[key]

    def hostile(self, va):
        return ()


class Gate(Module):
    """no float and no state: its bool, from every note script, among the votes of the layout"""
    mid, name, slots = GATE, "Gate", ()

    def ordinary(self, v):
        return [0.0]

    def variants(self):
        return [Variant()]

    def hostile(self, va):
        for k in range(len(NOTES)):
            yield dict(k=k, label=f"note script {k}", slot="note_on")


PCM_BYTES = F                      # the Sampler's one sample: mono s16, as many bytes as a column has floats (it rides in `cc2`)
SAMPLE_RATE_IN = 44100


class Sampler(Module):
    """sample_rate against the sample's own rate (ratio = 44100 / sample_rate; 0.9999 < ratio < 1.0001 plays without resampling);
    why no rate or play position can take a load out of the sample: tests/test_sample_kit_host.py"""
    mid, name, slots, state = SAMPLER, "Sampler", ("sample_rate",), ("t",)

    def ordinary(self, v):
        return [self.freq[v] * f32(40.0)]

    def columns(self, r, variant):
        r.cc2[:] = np.random.default_rng(4).integers(0, 256, PCM_BYTES).astype(f32)

    def variants(self):
        return [Variant(vi=(0,), label="once"), Variant(vi=(1,), label="looped")]

    def hostile(self, va):
        rin = f32(SAMPLE_RATE_IN)
        yield from self.slot_specs(va, "sample_rate", with_thresholds(rin, rin / f32(0.9999), rin / f32(1.0001), 0.0))
        yield from self.state_specs([[f32(x)] for x in (np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, -5.5, 1e9, 3e38, 170.0, 175.5)], "t")


class NoiseFilter(Module):
    """Noise -> Filter; every voice's generator starts from its own seed (p[7]), set as state on the device"""
    mid, name, slots = NOISEFILTER, "NoiseFilter", ("cutoff", "res")
    state = ("u:r0", "u:r1", "u:r2", "u:r3", "u:r4", "u:r5", "u:r6", "u:r7", "l", "b")

    def ordinary(self, v):
        return [0.02 + 0.5 * self.u2[v], 0.9 * self.u3[v]]

    def columns(self, r, variant):
        r.p[7] = f32(int(r.garbage.view(np.uint32)[0]) % 60000)

    def variants(self):
        return [Variant(vi=(c, t), label=f"{('white', 'pink')[c]}, {_FILTER_TYPES[t]}") for c in (0, 1) for t in (1, 4)]

    def hostile(self, va):
        yield from self.slot_specs(va, "cutoff", with_thresholds(0.0, 1.0))
        yield from self.slot_specs(va, "res", with_thresholds(0.0, 1.0))


class _Recipe(Module):
    """a script recipe as a generated kernel: hostile frequencies and every note script"""
    slots = ("freq",)

    def ordinary(self, v):
        return [self.freq[v]]

    def columns(self, r, variant):
        with np.errstate(over="ignore", invalid="ignore"):
            r.cctl *= r.p[0]

    def hostile(self, va):
        yield from self.slot_specs(va, "freq", with_thresholds(SR / 8, 0.0), "cctl" if va.vi[0] else None)
        for k in (3, 4):
            for x in (np.nan, 0.0, 1e9):
                yield dict(k=k, label=f"freq={x!r}, note script {k}", slot="pair", **(dict(img={"cctl": f32(x)}) if va.vi[0] else dict(repl={"freq": f32(x)})))


class FilteredSawtooth(_Recipe):
    mid, name = FSAW, "FilteredSawtooth"

    def variants(self):
        return [Variant(vi=(0,), label="constant"), Variant(vi=(1,), label="freq image")]


class HardSquare(_Recipe):
    mid, name = HSQUARE, "HardSquare"

    def variants(self):
        return [Variant(vi=(0,), label="constant")]


class StereoEchoes(FilteredEchoes):
    """the dry input to both outputs, a half delay into FilteredEchoes(main delay) to the left, a second half delay to the right.  The
    right output starts from the record's `cc2` column and is compared, with the three rings, as further state."""
    mid, name, state = STEREO, "StereoEchoes", ("u:index0", "u:index1", "u:index_e", "l", "b")


MODULES = {m.name: m for m in (SineOsc, PulseOsc, TriSawOsc, Cycle, Envelope, Portamento, Decimator, Distortion, Filter, NiceInstrument,
                               PMOscInstrument, FilteredEchoes, Curve, Gate, Sampler, NoiseFilter, FilteredSawtooth, HardSquare,
                               StereoEchoes)}
RECIPE_CUTOFF_HZ = 440.0           # examples/modules.zig:179-183: the recipe's filter sits at 440 Hz x note c5


def recipe_cutoff(oracle):
    L = oracle.lib()
    return float(L.zo_filter_cutoff_from_frequency(float(f32(RECIPE_CUTOFF_HZ) * f32(L.zo_note_c5())), SR))


def pcm_of(r):
    return np.ascontiguousarray(r.cc2[:PCM_BYTES].astype(np.uint8))


def noise_words(oracle, r):
    """the generator state of the record's seed: four uint64"""
    nz = oracle.Noise(); oracle.lib().zo_noise_init(C.byref(nz), int(r.p[7]))
    return [int(x) for x in nz.r]
_made = {}


def module(name):
    if name not in _made:
        _made[name] = MODULES[name]()
    return _made[name]


# ------------------------------------------------------------------------------------------ state words <-> bits
def st_bits(mod, st):
    """a record's state words as NST uint32"""
    out = np.zeros(NST, np.uint32)
    for i, (f, x) in enumerate(zip(mod.state, st)):
        out[i] = int(x) & 0xFFFFFFFF if f.startswith("u:") else bits(x)
    return out


# ------------------------------------------------------------------------------------------ the table as a file
def write_table(path, items):
    """items: [(module, variant, rec)] -> the file tests/cpp/hostile_oracle.c reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", MAGIC, len(items), F, len(SPANS)))
        for s, e in SPANS:
            f.write(struct.pack("<2I", s, e))
        for mod, va, r in items:
            f.write(struct.pack("<7I", mod.mid, *va.vi))
            f.write(np.asarray([va.sr], f32).tobytes())
            f.write(r.p.tobytes())
            f.write(struct.pack("<2I", r.k, 0 if r.st is None else 1))
            f.write((st_bits(mod, r.st) if r.st is not None else np.zeros(NST, np.uint32)).tobytes())
            for col in (r.garbage, r.cin, r.cctl, r.cc2):
                f.write(np.ascontiguousarray(col, f32).tobytes())


RESULT_WORDS = F + NST + NEX


def read_results(path, n):
    """-> (out [n][F] float32, states [n][NST] uint32, further state [n][NEX] float32) as the harness wrote them"""
    raw = np.fromfile(path, np.uint32)
    assert raw.size == n * RESULT_WORDS, (raw.size, n)
    raw = raw.reshape(n, RESULT_WORDS)
    return (np.ascontiguousarray(raw[:, :F]).view(f32), np.ascontiguousarray(raw[:, F:F + NST]),
            np.ascontiguousarray(raw[:, F + NST:]).view(f32))


# ------------------------------------------------------------------------------------------ the oracle, through ctypes
def reference(oracle, mod, va, r, batch=False):
    """the script of one voice through the oracle -> (out [F], state words [NST] uint32, further state [NEX]); kept on the record.
    `batch` (the oscillators): the second paint is the SECOND call of a paint_batch of two -- the same paint into another image first"""
    if batch:
        if r.ref_batch is None:
            keep = r.ref, r.ref_st, r.ref_ex
            r.ref = None
            r.ref_batch = _reference(oracle, mod, va, r, True)
            r.ref, r.ref_st, r.ref_ex = keep
        return r.ref_batch
    if r.ref is not None:
        return r.ref, r.ref_st, r.ref_ex
    return _reference(oracle, mod, va, r, False)


def _reference(oracle, mod, va, r, batch):
    L, o = oracle.lib(), oracle
    out = r.garbage.copy()
    sr, vi, p = float(va.sr), va.vi, [float(x) for x in r.p]
    cob = lambda is_img, col, x: o.buffer(col) if is_img else o.constant(x)
    words = []
    mid = mod.mid
    if mid == SINE:
        st = o.SineOsc(); L.zo_sineosc_init(C.byref(st))
        if r.st: st.t = r.st[0]
    elif mid == PULSE:
        st = o.PulseOsc(); L.zo_pulseosc_init(C.byref(st))
        if r.st: st.cnt = r.st[0]
    elif mid == TRISAW:
        st = o.TriSawOsc(); L.zo_trisawosc_init(C.byref(st))
        if r.st: st.cnt, st.t = r.st
    elif mid == CYCLE:
        st = o.Cycle(); L.zo_cycle_init(C.byref(st))
        if r.st: st.t = r.st[0]
    elif mid == ENVELOPE:
        st = o.Envelope(); L.zo_envelope_init(C.byref(st))
        if r.st: st.state, st.painter.t, st.painter.last_value, st.painter.start = r.st
    elif mid == PORTAMENTO:
        st = o.Portamento(); L.zo_portamento_init(C.byref(st))
        if r.st: st.painter.t, st.painter.last_value, st.painter.start = r.st
    elif mid == DECIMATOR:
        st = o.Decimator(); L.zo_decimator_init(C.byref(st))
        if r.st: st.dval, st.dcount = r.st
    elif mid == FILTER:
        st = o.Filter(); L.zo_filter_init(C.byref(st))
        if r.st: st.l, st.b = r.st
    elif mid == NICE:
        st = o.NiceInstrument(); L.zo_nice_init(C.byref(st), p[1])
        if r.st: st.osc.cnt, st.flt.l, st.flt.b, st.env.state, st.env.painter.t, st.env.painter.last_value, st.env.painter.start = r.st
    elif mid == PMOSC:
        st = o.PMOscInstrument(); L.zo_pmosc_init(C.byref(st), p[1])
        if r.st: st.carrier.t, st.modulator.t, st.env.state, st.env.painter.t, st.env.painter.last_value, st.env.painter.start = r.st
    elif mid == STEREO:
        st = o.Filter(); L.zo_filter_init(C.byref(st))
        H = MAIN_DELAY // 2
        ex = np.zeros(NEX, f32)
        right, r0, r1, re = ex[:F], ex[F:F + H], ex[F + H:F + 2 * H], ex[F + 2 * H:F + 2 * H + MAIN_DELAY]      # (views: contiguous)
        right[:] = r.cc2
        d0, d1, de = o.Delay(), o.Delay(), o.Delay()
        L.zo_delay_init(C.byref(d0), o.fptr(r0), H); L.zo_delay_init(C.byref(d1), o.fptr(r1), H); L.zo_delay_init(C.byref(de), o.fptr(re), MAIN_DELAY)
        t3 = np.zeros(F, f32)
    elif mid == SAMPLER:
        st = o.Sampler(); L.zo_sampler_init(C.byref(st))
        if r.st: st.t = r.st[0]
        pcm = pcm_of(r)
        sp = o.SamplerParams(p[0], 1, SAMPLE_RATE_IN, o.SAMPLE_S16, pcm.ctypes.data_as(C.POINTER(C.c_uint8)), pcm.size, 0, vi[0])
    elif mid == NOISEFILTER:
        st = o.Filter(); L.zo_filter_init(C.byref(st))
        nz = o.Noise(); L.zo_noise_init(C.byref(nz), int(r.p[7]))
    elif mid == FSAW:
        st = o.FilteredSawtooth(); L.zo_filtered_sawtooth_init(C.byref(st))
    elif mid == HSQUARE:
        st = o.HardSquare(); L.zo_hard_square_init(C.byref(st))
    elif mid == CURVE:
        st = o.CurveModule(); L.zo_curve_init(C.byref(st))
        n_nodes = int(r.p[0])
        carr = (o.CurveNode * max(n_nodes, 1))(*[o.CurveNode(float(r.cin[2 * j]), float(r.cin[2 * j + 1])) for j in range(n_nodes)])
    elif mid == ECHOES:
        st = o.Filter(); L.zo_filter_init(C.byref(st))
        ring = np.zeros(NEX, f32)
        dl = o.Delay(); L.zo_delay_init(C.byref(dl), o.fptr(ring), DELAY)
    extra = np.zeros(NEX, f32)
    t0, t1, t2 = (np.zeros(F, f32) for _ in range(3))
    prev_on = 0
    for i, (s, e) in enumerate(SPANS):
        if i == 0:
            L.zo_zero(s, e, o.fptr(out))
        nic, on = NOTES[r.k][i]
        if batch and i == 1:
            other = np.zeros(F, f32)
            (L.zo_pulseosc_paint if mid == PULSE else L.zo_trisawosc_paint)(C.byref(st), s, e, o.fptr(other), sr, cob(vi[0], r.cctl, p[0]), p[1])
        if mid == SINE:
            L.zo_sineosc_paint(C.byref(st), s, e, o.fptr(out), sr, cob(vi[0], r.cctl, p[0]), cob(vi[1], r.cin, p[1]))
        elif mid == PULSE:
            L.zo_pulseosc_paint(C.byref(st), s, e, o.fptr(out), sr, cob(vi[0], r.cctl, p[0]), p[1])
        elif mid == TRISAW:
            L.zo_trisawosc_paint(C.byref(st), s, e, o.fptr(out), sr, cob(vi[0], r.cctl, p[0]), p[1])
        elif mid == CYCLE:
            L.zo_cycle_paint(C.byref(st), s, e, o.fptr(out), sr, cob(vi[0], r.cctl, p[0]))
        elif mid == ENVELOPE:
            ep = o.EnvelopeParams(sr, o.curve(vi[0], p[0]), o.curve(vi[1], p[1]), o.curve(vi[2], p[2]), p[3], on)
            L.zo_envelope_paint(C.byref(st), s, e, o.fptr(out), nic, C.byref(ep))
        elif mid == PORTAMENTO:
            L.zo_portamento_paint(C.byref(st), s, e, o.fptr(out), nic, sr, o.curve(vi[0], p[0]), p[1], on, prev_on)
            prev_on = on
        elif mid == DECIMATOR:
            L.zo_decimator_paint(C.byref(st), s, e, o.fptr(out), sr, o.fptr(r.cin), p[0])
        elif mid == DISTORTION:
            L.zo_distortion_paint(s, e, o.fptr(out), o.fptr(r.cin), vi[0], p[0], p[1], p[2])
        elif mid == FILTER:
            L.zo_filter_paint(C.byref(st), s, e, o.fptr(out), o.fptr(r.cin), vi[0], cob(vi[1], r.cctl, p[0]), cob(vi[2], r.cc2, p[1]))
        elif mid == NICE:
            L.zo_nice_paint(C.byref(st), s, e, o.fptr(out), o.fptr(t0), o.fptr(t1), nic, sr, p[0], on)
        elif mid == PMOSC:
            L.zo_pmosc_paint(C.byref(st), s, e, o.fptr(out), o.fptr(t0), o.fptr(t1), o.fptr(t2), nic, sr, p[0], on)
        elif mid == ECHOES:
            L.zo_filtered_echoes_paint(C.byref(dl), C.byref(st), s, e, o.fptr(out), o.fptr(t0), o.fptr(t1), o.fptr(r.cin), p[0], p[1])
        elif mid == CURVE:
            L.zo_curve_paint(C.byref(st), s, e, o.fptr(out), nic, sr, vi[0], carr, n_nodes)
        elif mid == STEREO:                                  # examples/modules.zig:503-522
            if i == 0:
                L.zo_zero(s, e, o.fptr(right))
            L.zo_add_into(s, e, o.fptr(out), o.fptr(r.cin)); L.zo_add_into(s, e, o.fptr(right), o.fptr(r.cin))
            L.zo_zero(s, e, o.fptr(t0)); L.zo_simple_delay_paint(C.byref(d0), s, e, o.fptr(t0), o.fptr(r.cin))
            L.zo_zero(s, e, o.fptr(t1))
            L.zo_filtered_echoes_paint(C.byref(de), C.byref(st), s, e, o.fptr(t1), o.fptr(t2), o.fptr(t3), o.fptr(t0), p[0], p[1])
            L.zo_add_into(s, e, o.fptr(out), o.fptr(t1))
            L.zo_simple_delay_paint(C.byref(d1), s, e, o.fptr(right), o.fptr(t1))
        elif mid == GATE:
            L.zo_gate_paint(s, e, o.fptr(out), on)
        elif mid == SAMPLER:
            L.zo_sampler_paint(C.byref(st), s, e, o.fptr(out), nic, C.byref(sp))
        elif mid == NOISEFILTER:
            L.zo_zero(s, e, o.fptr(t0))
            L.zo_noise_paint(C.byref(nz), s, e, o.fptr(t0), vi[0])
            L.zo_filter_paint(C.byref(st), s, e, o.fptr(out), o.fptr(t0), vi[1], o.constant(p[0]), o.constant(p[1]))
        elif mid == FSAW:
            L.zo_filtered_sawtooth_paint(C.byref(st), s, e, o.fptr(out), o.fptr(t0), o.fptr(t1), o.fptr(t2), nic, sr, cob(vi[0], r.cctl, p[0]), on)
        elif mid == HSQUARE:
            L.zo_hard_square_paint(C.byref(st), s, e, o.fptr(out), o.fptr(t0), o.fptr(t1), nic, sr, p[0], on)
    if mid == SINE or mid == CYCLE:
        words = [st.t]
    elif mid == PULSE:
        words = [st.cnt]
    elif mid == TRISAW:
        words = [st.cnt, st.t]
    elif mid == ENVELOPE:
        words = [st.state, st.painter.t, st.painter.last_value, st.painter.start]
    elif mid == PORTAMENTO:
        words = [st.painter.t, st.painter.last_value, st.painter.start]
    elif mid == DECIMATOR:
        words = [st.dval, st.dcount]
    elif mid == FILTER:
        words = [st.l, st.b]
    elif mid == NICE:
        words = [st.osc.cnt, st.flt.l, st.flt.b, st.env.state, st.env.painter.t, st.env.painter.last_value, st.env.painter.start]
    elif mid == PMOSC:
        words = [st.carrier.t, st.modulator.t, st.env.state, st.env.painter.t, st.env.painter.last_value, st.env.painter.start]
    elif mid == CURVE:
        words = [st.t, st.current_song_note, st.current_song_note_offset, st.next_song_note]
    elif mid == STEREO:
        words = [d0.index, d1.index, de.index, st.l, st.b]
        extra = ex
    elif mid == SAMPLER:
        words = [st.t]
    elif mid == NOISEFILTER:
        words = [w for x in nz.r for w in (int(x) & 0xFFFFFFFF, int(x) >> 32)] + [st.l, st.b]
    elif mid == ECHOES:
        words = [dl.index, st.l, st.b]
        extra = ring
    r.ref, r.ref_st, r.ref_ex = out, st_bits(mod, words), extra
    return r.ref, r.ref_st, r.ref_ex


# ------------------------------------------------------------------------------------------ the comparison
def same_f32(a, b):
    """bit for bit (the sign of a zero and of an infinity included), except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def first_difference(a, b):
    """(index, a there, b there) of the first element that same_f32 tells apart, or None"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    w = np.argwhere(bad)
    if not len(w):
        return None
    i = tuple(int(x) for x in w[0])
    return i, a[i], b[i], int(bad.sum())


def float_state_mask(mod):
    return np.array([not f.startswith("u:") for f in mod.state] + [False] * (NST - len(mod.state)))


def same_state(mod, got, want):
    """state words [.., NST] uint32: integer words equal outright, float words as same_f32"""
    fm = float_state_mask(mod)
    n = len(mod.state)
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    ints = np.array_equal(got[..., :n][..., ~fm[:n]], want[..., :n][..., ~fm[:n]])
    return ints and same_f32(np.ascontiguousarray(got[..., :n][..., fm[:n]]).view(f32), np.ascontiguousarray(want[..., :n][..., fm[:n]]).view(f32))


# ------------------------------------------------------------------------------------------ the device
def _image(cols):
    """[voices][F] host columns -> a CUDA image [F][voices]"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(cols).T)).cuda()


_PROGRAMS = {}


def recipe_program(ctx, name, roles):
    """the script recipe `name` of tests/golden/script_modules.txt, compiled once per form set (roles: with the role-wave kernel)"""
    import os
    from zang_amd import script, zscript_native as native
    key = (name, bool(roles))
    if key not in _PROGRAMS:
        text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "script_modules.txt")).read()
        _PROGRAMS[key] = script.ScriptProgram(text, ctx, only=[name], forms=native.FORM_ROLES if roles else native.FORM_ROLES_WORTH)
    return _PROGRAMS[key]


def paint_device(ctx, mod, va, recs, unchanged=False, batch=False, oracle=None, roles=False):
    """The script of a chunk on the device -> (out [voices][F], state words [voices][NST] uint32, the kernels every paint
    launched).  `unchanged` (the oscillators): the paints after the first state ZH_PAINT_PARAMS_UNCHANGED.  `batch` (the
    oscillators): the second paint is a paint_batch of two images, another image first and the output second.  `oracle`: for the
    modules whose set-up needs it (a NoiseFilter voice's generator state, the recipes' cutoff); `roles` (the script recipes): the
    program compiled with its role-wave kernel."""
    import torch
    from zang_amd import modules as M, zang
    n = len(recs)
    P = np.stack([r.p for r in recs])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    col = [dev(P[:, j]) for j in range(NP)]
    sr, vi, mid = float(va.sr), va.vi, mod.mid
    cin = _image([r.cin for r in recs]) if mid in (SINE, DECIMATOR, DISTORTION, FILTER, ECHOES, STEREO) else None
    cctl = _image([r.cctl for r in recs]) if mid in (SINE, PULSE, TRISAW, CYCLE, FILTER, FSAW) else None
    cc2 = _image([r.cc2 for r in recs]) if mid in (FILTER, STEREO) else None            # (StereoEchoes: the right output)
    out = _image([r.garbage for r in recs])
    cob = lambda is_img, img, j: zang.buffer(img) if is_img else zang.constant(col[j])
    cls = {SINE: M.SineOsc, PULSE: M.PulseOsc, TRISAW: M.TriSawOsc, CYCLE: M.Cycle, ENVELOPE: M.Envelope, PORTAMENTO: M.Portamento,
           DECIMATOR: M.Decimator, DISTORTION: M.Distortion, FILTER: M.Filter}.get(mid)
    if mid == NICE:
        m = M.NiceInstrument(n, col[1], ctx)
    elif mid == PMOSC:
        m = M.PMOscInstrument(n, col[1], ctx)
    elif mid == ECHOES:
        m = M.FilteredEchoes(n, DELAY, ctx)
    elif mid == CURVE:
        m = M.Curve(n, ctx)
        n_nodes = int(recs[0].p[0])
        nodes = dev(recs[0].cin[:2 * n_nodes].reshape(n_nodes, 2).copy())
    elif mid == STEREO:
        m = M.StereoEchoes(n, MAIN_DELAY, ctx)
    elif mid == GATE:
        m = M.Gate(n, ctx)
    elif mid == SAMPLER:
        m = M.Sampler(n, ctx)
        pcm = dev(pcm_of(recs[0]))
        smp = m.Sample(1, SAMPLE_RATE_IN, m.signed16_lsb, pcm)
    elif mid == NOISEFILTER:
        m = M.NoiseFilter(n, ctx)
        st = m.state()
        for v, r in enumerate(recs):
            st["noise"]["r"][v] = noise_words(oracle, r)
        m.set_state(st)
    elif mid in (FSAW, HSQUARE):
        script_name = "HardSquare" if mid == HSQUARE else ("FilteredSawtoothCtl" if vi[0] else "FilteredSawtooth")
        m = recipe_program(ctx, script_name, roles).module(script_name, n)
    else:
        m = cls(n, ctx)
    names = [] if mid == NOISEFILTER else [f[2:] if f.startswith("u:") else f for f in mod.state]

    def field(st, f):
        for part in f.split("."):
            st = st[part]
        return st
    if any(r.st is not None for r in recs):
        st = m.state()
        for v, r in enumerate(recs):
            if r.st is not None:
                for f, x in zip(names, r.st):
                    field(st, f)[v] = x
        m.set_state(st)
    notes = np.array([NOTES[r.k] for r in recs], np.uint8)                          # [voices][paint][nic, on]
    keep, forms = [], []
    for i, (s, e) in enumerate(SPANS):
        span, zf, kw = zang.Span(s, e), i == 0, {}
        nic, on = dev(notes[:, i, 0]), dev(notes[:, i, 1])
        prev = dev(notes[:, i - 1, 1]) if i else dev(np.zeros(n, np.uint8))
        keep += [nic, on, prev]
        if mid == SINE:
            p = m.Params(sr, cob(vi[0], cctl, 0), cob(vi[1], cin, 1))
        elif mid in (PULSE, TRISAW):
            p = m.Params(sr, cob(vi[0], cctl, 0), col[1])
            kw = dict(params_unchanged=unchanged and i > 0)
        elif mid == CYCLE:
            p = m.Params(sr, cob(vi[0], cctl, 0))
        elif mid == ENVELOPE:
            p = m.Params(sr, zang.PaintCurve._mk(vi[0], col[0]), zang.PaintCurve._mk(vi[1], col[1]), zang.PaintCurve._mk(vi[2], col[2]), col[3], on)
        elif mid == PORTAMENTO:
            p = m.Params(sr, zang.PaintCurve._mk(vi[0], col[0]), col[1], on, prev)
        elif mid == DECIMATOR:
            p = m.Params(sr, cin, col[0])
        elif mid == DISTORTION:
            p = m.Params(cin, vi[0], col[0], col[1], col[2])
        elif mid == FILTER:
            p = m.Params(cin, vi[0], cob(vi[1], cctl, 0), cob(vi[2], cc2, 1))
        elif mid in (NICE, PMOSC):
            p = m.Params(sr, col[0], on)
        elif mid == ECHOES:
            p = m.Params(cin, col[0], col[1])
        elif mid == CURVE:
            p = m.Params(sr, vi[0], nodes)
        elif mid == STEREO:
            p = m.Params(cin, col[0], col[1])
        elif mid == GATE:
            p = m.Params(on)
        elif mid == SAMPLER:
            p = m.Params(col[0], smp, 0, bool(vi[0]))
        elif mid == NOISEFILTER:
            p = m.Params(vi[0], vi[1], col[0], col[1])
        elif mid in (FSAW, HSQUARE):
            p = {"sample_rate": sr, "freq": cctl if (mid == FSAW and vi[0]) else col[0], "note_on": on}
            if mid == FSAW:
                p["cutoff"] = recipe_cutoff(oracle)
        if mid == STEREO:
            m.paint(span, [out, cc2], None, False, p, zero_first=zf)
        elif batch and i == 1:
            other = torch.zeros_like(out)
            keep.append(other)
            m.paint_batch(span, [other, out], p, zero_first=zf, **kw)
        else:
            m.paint(span, [out], None if mid in (NICE, PMOSC, ECHOES, NOISEFILTER, FSAW, HSQUARE) else [],
                    nic if mid in (ENVELOPE, PORTAMENTO, NICE, PMOSC, CURVE, SAMPLER, FSAW, HSQUARE) else False, p, zero_first=zf, **kw)
        forms.append(ctx.last_form())
    ctx.sync()
    got = np.ascontiguousarray(out.cpu().numpy().T)
    words = np.zeros((n, NST), np.uint32)
    extra = np.zeros((n, NEX), f32)
    if mid == ECHOES:
        rings, index, flt = m.state()
        extra[:, :DELAY] = rings
        words[:, 0] = index
        words[:, 1] = np.ascontiguousarray(flt["l"].astype(f32)).view(np.uint32)
        words[:, 2] = np.ascontiguousarray(flt["b"].astype(f32)).view(np.uint32)
    elif mid == STEREO:
        g0, i0, g1, i1, ge, ie, flt = m.state()
        H = MAIN_DELAY // 2
        extra[:, :F] = cc2.cpu().numpy().T
        extra[:, F:F + H] = g0; extra[:, F + H:F + 2 * H] = g1; extra[:, F + 2 * H:F + 2 * H + MAIN_DELAY] = ge
        words[:, 0], words[:, 1], words[:, 2] = i0, i1, ie
        words[:, 3] = np.ascontiguousarray(flt["l"].astype(f32)).view(np.uint32)
        words[:, 4] = np.ascontiguousarray(flt["b"].astype(f32)).view(np.uint32)
    elif mid == NOISEFILTER:
        st = m.state()
        r = np.asarray(st["noise"]["r"]).astype(np.uint64)                   # [voices][4]
        for j in range(4):
            words[:, 2 * j] = (r[:, j] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            words[:, 2 * j + 1] = (r[:, j] >> np.uint64(32)).astype(np.uint32)
        words[:, 8] = np.ascontiguousarray(st["flt"]["l"].astype(f32)).view(np.uint32)
        words[:, 9] = np.ascontiguousarray(st["flt"]["b"].astype(f32)).view(np.uint32)
    elif names:
        st = m.state()
        for j, (f, full) in enumerate(zip(names, mod.state)):
            a = np.asarray(field(st, f))
            words[:, j] = a.astype(np.int64).astype(np.uint32) if full.startswith("u:") else np.ascontiguousarray(a.astype(f32)).view(np.uint32)
    m.close()
    return got, words, extra, forms


def compare_chunk(oracle, mod, va, recs, got, words, extra, what, batch=False):
    """every checked voice of a chunk against the oracle -> (voices compared, hostile voices compared, NaN samples, samples)"""
    idx = mod.checked(va, recs)
    ref = np.stack([reference(oracle, mod, va, recs[i], batch)[0] for i in idx])
    ref_st = np.stack([reference(oracle, mod, va, recs[i], batch)[1] for i in idx])
    ref_ex = np.stack([reference(oracle, mod, va, recs[i], batch)[2] for i in idx])
    d = first_difference(got[idx], ref)
    if d is not None:
        (j, f), g, w, nbad = d
        r = recs[idx[j]]
        raise AssertionError(f"{what} [{va!r}]: {nbad} samples differ, first at voice {idx[j]} ({r.label}; p={list(r.p[:len(mod.slots)])}, state {r.st}, "
                             f"notes {r.k}) frame {f}: device {g!r} ({bits(g):#010x}), oracle {w!r} ({bits(w):#010x})")
    for j, i in enumerate(idx):
        if not same_state(mod, words[i], ref_st[j]):
            r = recs[i]
            raise AssertionError(f"{what} [{va!r}]: state of voice {i} ({r.label}; p={list(r.p[:len(mod.slots)])}, state {r.st}, notes {r.k}): "
                                 f"device {[hex(x) for x in words[i]]}, oracle {[hex(x) for x in ref_st[j]]}")
    d = first_difference(extra[idx], ref_ex)
    if d is not None:
        (j, f), g, w, nbad = d
        raise AssertionError(f"{what} [{va!r}]: {nbad} further state words (a delay ring) differ, first at voice {idx[j]} ({recs[idx[j]].label}) word {f}: "
                             f"device {g!r}, oracle {w!r}")
    hostile = [j for j, i in enumerate(idx) if recs[i].hostile or va.shared_by_paint]
    return len(idx), len(hostile), int(np.isnan(ref[hostile]).sum()), int(ref[hostile].size)
