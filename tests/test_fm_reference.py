"""CPU: tests/fm_reference.py -- the np.float32 restatement of examples/example_fmsynth.zig:22-356 the GPU tests compare with --
pinned to the committed oracle, and the GPU corpus (tests/fm_cases.py) checked for what it covers.  Bit for bit throughout."""
import ctypes as C
import math

import numpy as np

from oracle import pyoracle as po
from tests import fm_cases as fc
from tests import fm_reference as fr
from tests.util import assert_bitexact

F32 = np.float32
SR = 48000.0
CHAIN = fc.CHAIN


def _patch(**kw):
    p = list(fr.DEFAULT_PATCH)
    for k, v in kw.items():
        p[getattr(fr, k)] = v
    return tuple(p)


# ------------------------------------------------------------------ 1. the helper is the oracle's composition
def _oracle_operator(L, osc, env, s, e, out, t0, t1, nic, freq, note_on, k, phase, trem, vib):
    """Operator.paint (:205-240) as calls of the oracle's buffer operations, SineOsc and Envelope"""
    L.zo_zero(s, e, po.fptr(t1))
    L.zo_multiply_scalar(s, e, po.fptr(t1), po.fptr(vib), float(k["vibrato"]))
    L.zo_add_scalar_into(s, e, po.fptr(t1), 1.0)
    L.zo_multiply_with_scalar(s, e, po.fptr(t1), float(F32(freq) * k["freq_mul"]))
    L.zo_zero(s, e, po.fptr(t0))
    L.zo_sineosc_paint(C.byref(osc), s, e, po.fptr(t0), SR, po.buffer(t1), po.buffer(phase) if phase is not None else po.constant(0.0))
    L.zo_multiply_with_scalar(s, e, po.fptr(t0), float(k["volume"]))
    L.zo_zero(s, e, po.fptr(t1))
    L.zo_multiply_scalar(s, e, po.fptr(t1), po.fptr(trem), float(k["tremolo"]))
    L.zo_add_scalar_into(s, e, po.fptr(t1), 1.0)
    L.zo_multiply_with(s, e, po.fptr(t0), po.fptr(t1))
    L.zo_zero(s, e, po.fptr(t1))
    prm = po.EnvelopeParams(SR, po.curve(po.CURVE_CUBED, k["attack"]), po.curve(po.CURVE_CUBED, k["decay"]), po.curve(po.CURVE_CUBED, k["release"]),
                            float(k["sustain"]), 1 if note_on else 0)
    L.zo_envelope_paint(C.byref(env), s, e, po.fptr(t1), 1 if nic else 0, C.byref(prm))
    L.zo_multiply(s, e, po.fptr(out), po.fptr(t0), po.fptr(t1))


def test_without_feedback_the_helper_is_the_oracles_sineosc_composition():
    """Feedback 0 and waveform 0: the Oscillator is SineOsc on its buffer-frequency path with a phase buffer.  Eight voices -- both
    algorithms x tremolo x vibrato, unequal operator settings -- over the chain of spans with the notes going on, off and on again:
    outputs, oscillator phases (the end-of-span wrap) and envelope states equal the composition of the oracle's own calls."""
    L = po.lib()
    F = 1024
    pats = [_patch(ALGORITHM=a, MOD_TREMOLO=t, CAR_TREMOLO=1 - t, MOD_VIBRATO=v, CAR_VIBRATO=v, TREMOLO_DEPTH=t, VIBRATO_DEPTH=1 - v,
                   MOD_FREQ_MUL=(0, 3, 11, 15)[2 * t + v], CAR_VOLUME=5 * v, MOD_VOLUME=33 * t, MOD_ATTACK=15, CAR_ATTACK=14, MOD_DECAY=15,
                   CAR_DECAY=13, MOD_SUSTAIN=3, CAR_RELEASE=13, MOD_RELEASE=15)
            for a in (0, 1) for t in (0, 1) for v in (0, 1)]
    V = len(pats)
    rng = np.random.default_rng(5)
    freq = rng.uniform(100.0, 3000.0, V).astype(F32)
    trem = (0.9 * np.sin(np.arange(F) * 0.01 + np.arange(V)[:, None])).astype(F32)
    vib = (0.8 * np.cos(np.arange(F) * 0.013 + np.arange(V)[:, None])).astype(F32)
    live = rng.uniform(-1, 1, (V, F)).astype(F32)
    on = [(True, True), (False, False), (True, True), (True, False)]           # (note_on, note_id_changed) per paint of the chain
    ref = fr.FMRef(V, 1, pats)
    got = live.copy()
    want = live.copy()
    oscs = [[po.SineOsc(), po.SineOsc()] for _ in range(V)]
    envs = [[po.Envelope(), po.Envelope()] for _ in range(V)]
    for v in range(V):
        for op in range(2):
            L.zo_sineosc_init(C.byref(oscs[v][op])); L.zo_envelope_init(C.byref(envs[v][op]))
    t0, t1, t2 = (np.zeros(F, F32) for _ in range(3))
    for (s, e), (note_on, nic) in zip(CHAIN, on):
        ref.paint_into(got, s, e, nic, SR, trem, vib, freq, note_on)
        for v in range(V):
            m, c, _, _, alg = fr.patch_constants(pats[v])
            if alg == 0:                                                       # :300-304
                _oracle_operator(L, oscs[v][0], envs[v][0], s, e, want[v], t1, t2, nic, freq[v], note_on, m, None, trem[v], vib[v])
                phase = None
            else:                                                              # :305-310
                L.zo_zero(s, e, po.fptr(t0))
                _oracle_operator(L, oscs[v][0], envs[v][0], s, e, t0, t1, t2, nic, freq[v], note_on, m, None, trem[v], vib[v])
                phase = t0
            _oracle_operator(L, oscs[v][1], envs[v][1], s, e, want[v], t1, t2, nic, freq[v], note_on, c, phase, trem[v], vib[v])
        assert_bitexact(got, want, f"span {(s, e)}")
        st = ref.state()
        for op in range(2):
            assert_bitexact(st["t"][:, op], np.array([oscs[v][op].t for v in range(V)], F32), f"t, span {(s, e)}")
            for v in range(V):
                env = envs[v][op]
                assert (st[v, op]["env_state"], st[v, op]["env_t"].tobytes(), st[v, op]["env_last_value"].tobytes(), st[v, op]["env_start"].tobytes()) == \
                    (env.state, F32(env.painter.t).tobytes(), F32(env.painter.last_value).tobytes(), F32(env.painter.start).tobytes())
    assert np.abs(want - live).max() > 0.1 and (ref.t > 0).all()


def test_waveforms_are_functions_of_the_same_argument():
    """With feedback 0 the modulator's sine argument does not depend on the waveform: waveforms 1-3 see the arguments waveform 0 sees, and
    their samples are max(s, 0), |s| and |s| gated by the sign of sin(2p) (:75-80) of the oracle's sines."""
    F = 512
    trem, vib = np.zeros((4, F), F32), np.zeros((4, F), F32)
    ref = fr.FMRef(4, 1, [_patch(MOD_WAVEFORM=w, ALGORITHM=0, CAR_WAVEFORM=3 - w) for w in range(4)])
    ref.paint(0, F, True, SR, trem, vib, 1234.5, True)
    for op in range(2):
        p, smp = ref.last_p[op], ref.last_samples[op]
        waves = [w if op == 0 else 3 - w for w in range(4)]
        for r in range(1, 4):
            assert_bitexact(p[r], p[0], f"operator {op}: the arguments of voice {r}")
        s = np.array([[po.lib().zo_math_sinf(float(x)) for x in p[0]]], F32)[0]
        s2 = np.array([[po.lib().zo_math_sinf(float(F32(x) * F32(2))) for x in p[0]]], F32)[0]
        want = {0: s, 1: np.maximum(s, F32(0)), 2: np.abs(s), 3: np.where(s2 >= 0, np.abs(s), F32(0)).astype(F32)}
        for r, w in enumerate(waves):
            assert_bitexact(smp[r], want[w], f"operator {op}, waveform {w}")
        assert (s < 0).any() and (s2 < 0).any() and ((s2 < 0) != (s < 0)).any()


def test_feedback_is_a_recurrence_through_the_sine():
    """the modulator's own last two samples reach its phase (:71-73, :85-86): restated frame by frame with scalar oracle calls"""
    F = 64
    z = np.zeros((1, F), F32)
    ref = fr.FMRef(1, 1, [_patch(MOD_FEEDBACK=7, MOD_WAVEFORM=3, ALGORITHM=0)])
    ref.paint(0, F, True, SR, z, z, 997.0, True)
    L = po.lib()
    t, fb1, fb2 = F32(0), F32(0), F32(0)
    step = (F32(0) + F32(0) * F32(0) + F32(1)) * (F32(997.0) * F32(2.0)) * (F32(1) / F32(SR))
    for i in range(F):
        p = (t + F32(0)) * fr.PI * F32(2) + (fb1 + fb2) * fr.FEEDBACK[7]
        s, s2 = F32(L.zo_math_sinf(float(p))), F32(L.zo_math_sinf(float(p * F32(2))))
        smp = F32(abs(s)) if s2 >= 0 else F32(0)
        assert ref.last_p[0][0, i].tobytes() == F32(p).tobytes() and ref.last_samples[0][0, i].tobytes() == smp.tobytes(), i
        t, fb2, fb1 = t + step, fb1, smp
    assert ref.fb1[0][0].tobytes() == fb1.tobytes() and ref.fb2[0][0].tobytes() == fb2.tobytes()


# ------------------------------------------------------------------ 2. patch constants
def test_patch_constants():
    from zang_amd import abi
    # the default patch is :376-397, and the library's zh_fm_patch_default agrees
    assert fr.DEFAULT_PATCH == (2, 0, 0, 8, 8, 1, 8, 0, 0, 0, 1, 0, 0, 8, 8, 1, 8, 0, 0, 1, 1, 1)
    assert fr.NUM_VALUES == (16, 4, 64, 16, 16, 16, 16, 2, 2, 8, 16, 4, 64, 16, 16, 16, 16, 2, 2, 2, 2, 2)
    p = abi.FMPatch()
    assert abi.load().zh_fm_patch_default(C.byref(p)) == 0 and tuple(p.value) == fr.DEFAULT_PATCH
    assert abi.load().zh_fm_patch_default(None) == abi.ZH_ERR_INVALID
    k = lambda **kw: fr.op_constants(**{**dict(freq_mul=1, volume=0, attack=8, decay=8, sustain=0, release=8, tremolo=0, vibrato=0,
                                               tremolo_depth=0, vibrato_depth=0), **kw})
    assert k()["volume"] == F32(1.0) and k()["sustain"] == F32(1.0)            # index 0: pow(10, 0) is exactly 1
    assert [float(k(freq_mul=i)["freq_mul"]) for i in range(16)] == [0.5, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 12, 12, 15, 15]
    assert [x.tobytes() for x in fr.FEEDBACK] == [F32(x).tobytes() for x in (0, math.pi / 16, math.pi / 8, math.pi / 4, math.pi / 2, math.pi,
                                                                             2 * math.pi, 4 * math.pi)]
    L = po.lib()
    pw = lambda x, y: F32(L.zo_math_powf(float(F32(x)), float(F32(y))))
    assert k(volume=63)["volume"].tobytes() == pw(10, F32(-47.25) / F32(20)).tobytes()
    assert k(sustain=15)["sustain"].tobytes() == pw(10, F32(-45.0) / F32(20)).tobytes()
    assert k(attack=15)["attack"] == F32(0.002) and k(attack=0)["attack"] == F32(0.002) + F32(4.0)
    assert k(decay=8)["decay"].tobytes() == (F32(0.002) + F32(4.0) * pw(F32(1) - F32(8) / F32(15), 3)).tobytes()
    assert k(tremolo=1, tremolo_depth=1)["tremolo"].tobytes() == (F32(1) - pw(10, F32(-4.8) / F32(20))).tobytes()
    assert k(vibrato=1, vibrato_depth=0)["vibrato"].tobytes() == (pw(2, F32(7 / 1200)) - F32(1)).tobytes()
    assert k(vibrato=1, vibrato_depth=1)["vibrato"].tobytes() == (pw(2, F32(14 / 1200)) - F32(1)).tobytes()
    assert k(tremolo=0, tremolo_depth=1)["tremolo"] == 0 and k(vibrato=0, vibrato_depth=1)["vibrato"] == 0


# ------------------------------------------------------------------ 3. what the GPU corpus covers
def test_the_gpu_corpus_covers_every_axis():
    pats = np.array(fc.patches())
    assert pats.shape == (fc.NI, 22) and (pats < np.array(fr.NUM_VALUES)).all()
    col = lambda name: set(pats[:, getattr(fr, name)].tolist())
    assert col("MOD_WAVEFORM") == col("CAR_WAVEFORM") == {0, 1, 2, 3}
    assert col("MOD_FEEDBACK") == set(range(8)) and col("ALGORITHM") == {0, 1}
    for op in ("MOD", "CAR"):
        assert {0, 10, 11, 12, 13, 14, 15} <= col(op + "_FREQ_MUL")
        for name in ("ATTACK", "DECAY", "RELEASE"):
            assert {0, 15} <= col(f"{op}_{name}"), (op, name)
    trem = {(int(p[fr.MOD_TREMOLO]) | int(p[fr.CAR_TREMOLO]), int(p[fr.TREMOLO_DEPTH])) for p in pats}
    vib = {(int(p[fr.MOD_VIBRATO]) | int(p[fr.CAR_VIBRATO]), int(p[fr.VIBRATO_DEPTH])) for p in pats}
    assert {(1, 0), (1, 1)} <= trem and {(1, 0), (1, 1)} <= vib and any(t == 0 for t, _ in trem) and any(v == 0 for v, _ in vib)
    vol = np.bitwise_or.reduce(pats[:, fr.MOD_VOLUME]) | np.bitwise_or.reduce(pats[:, fr.CAR_VOLUME])
    sus = np.bitwise_or.reduce(pats[:, fr.MOD_SUSTAIN]) | np.bitwise_or.reduce(pats[:, fr.CAR_SUSTAIN])
    assert vol == 63 and sus == 15
    x, ref = fc.inputs(), fc.reference()
    assert x["freq"][fc.ZERO_HZ_VOICE] == 0 and x["on"][:, fc.ZERO_HZ_VOICE].any() and not x["on"][:, fc.SILENT_VOICE].any()
    assert (ref["classes"] > 0).all(), ref["classes"]                          # every |p| class, modulator and carrier
    assert ref["stages"] == {po.ENV_IDLE, po.ENV_ATTACK, po.ENV_DECAY, po.ENV_SUSTAIN, po.ENV_RELEASE}
    retriggered = [ref["release_at"][k] & x["on"][k] & x["nic"][k] for k in range(len(fc.CHAIN))]
    assert any(r.any() for r in retriggered), "no note re-triggered mid-release"
    silent = np.concatenate([p["c"][fc.SILENT_VOICE] for p in ref["paints"]])
    assert not silent.any() and all(np.abs(p["c"]).max() > 0.05 for p in ref["paints"])
    # the span corpus: 0-3 sub-spans, touching ones, one that ends with the buffer, a single frame; its three buffers carry sound
    counts = {int(c) for tb in fc.span_tables() for c in tb["count"]}
    assert counts == {0, 1, 2, 3}
    assert all(np.abs(c).max() > 0.05 and painted.any() and not painted.all() for _, c, painted, _, _ in fc.span_reference())
