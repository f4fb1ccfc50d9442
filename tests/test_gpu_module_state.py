"""GPU: create / state() / set_state() of the ten builtin modules whose state is one [words][n] block (SineOsc, Sampler, Cycle,
PulseOsc, Envelope, Portamento, Decimator, Curve, PMOscInstrument: double-buffered zh_flipper blocks; FMInstrument: one block), whose
host side is csrc/state_block.hip.h over the Layouts of module_state.hip.h and fm.hip.h.  At n = 0, 1, 65 and 130 voices:

  a fresh module's state() is the reference's init() (the oracle's zo_<module>_init where it has one): every word zero, but the
  Decimator's dcount = 1;
  set_state(hostile) then state() gives the same BITS back: NaN payloads, -0.0, denormals, 0xFFFFFFFF, negative
  current_song_note_offset (FM's `reserved` is no state: it reads back 0 whatever was set);
  NULL pointers are ZH_ERR_INVALID.

And for the six modules that have a frame-range form, which reads one buffer and writes the OTHER (the host flips): at 333 voices
and 1,024 frames with the form's dispatch row at 2 ranges (what tests/test_gpu_dispatch.py
test_forced_large_voice_count_geometries_at_a_small_voice_count pins) one span is painted -- the range kernel is checked to have
run -- and then state() / set_state() must address the buffer the next paint starts from: the hostile round trip again; an empty
span leaves the state alone (PulseOsc: whatever the state; the others: from the state the paint left, same params, no new note --
the reference's prologues change nothing then and SineOsc's `t -= trunc(t)` is idempotent); and a second range paint from the
restored state gives the image and the state of a module that was painted twice and never read.
"""
import ctypes as C

import numpy as np
import pytest

from tests import util
from tests.test_gpu_views import _clear_env

pytestmark = pytest.mark.gpu
SR = 48000.0
NS = [0, 1, 65, 130]
V, F = 333, 1024                        # tests/test_gpu_dispatch.py: FORCED's voice count, _shared's span (0, 1024)


def _mods():
    from zang_amd import modules as mod
    # name -> (class, create arguments after n, the oracle's struct and init (None: no such module there; init() is all zero))
    return {
        "sineosc": (mod.SineOsc, (), ("SineOsc", "zo_sineosc_init", ())),
        "sampler": (mod.Sampler, (), ("Sampler", "zo_sampler_init", ())),
        "cycle": (mod.Cycle, (), ("Cycle", "zo_cycle_init", ())),
        "pulseosc": (mod.PulseOsc, (), ("PulseOsc", "zo_pulseosc_init", ())),
        "envelope": (mod.Envelope, (), ("Envelope", "zo_envelope_init", ())),
        "portamento": (mod.Portamento, (), ("Portamento", "zo_portamento_init", ())),
        "decimator": (mod.Decimator, (), ("Decimator", "zo_decimator_init", ())),
        "curve": (mod.Curve, (), ("CurveModule", "zo_curve_init", ())),
        "pmosc": (mod.PMOscInstrument, (0.25,), ("PMOscInstrument", "zo_pmosc_init", (C.c_float(0.25),))),
        "fm": (mod.FMInstrument, (), None),
    }


NAMES = ["sineosc", "sampler", "cycle", "pulseosc", "envelope", "portamento", "decimator", "curve", "pmosc", "fm"]


def _make(name, n, ctx):
    cls, args, _ = _mods()[name]
    return cls(n, *args, ctx) if name == "pmosc" else cls(n, ctx)


def _leaves_ctypes(st, skip=("release_duration",)):
    out = []
    for f in st._fields_:
        v = getattr(st, f[0])
        if f[0] in skip:
            continue
        out += _leaves_ctypes(v, skip) if isinstance(v, C.Structure) else [v]
    return out


def _leaves_numpy(row):
    out = []
    for f in row.dtype.names:
        out += _leaves_numpy(row[f]) if row[f].dtype.names else [row[f].item()]
    return out


_PATTERNS = np.array([0x7FC00001, 0x80000000, 0x00000001, 0xFFFFFFFF, 0x7F800001, 0x807FFFFF, 0xFFC12345, 0x007FFFFF], np.uint32)


def _hostile(m, seed):
    """n states of the module's struct from raw words: the fixed patterns (quiet and signalling NaNs with payloads, -0.0, denormals,
    all ones) down the diagonals, random bits elsewhere"""
    dt = np.dtype(m._state_ctype)
    n, words = m.n_voices, dt.itemsize // 4
    w = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, words), dtype=np.uint64).astype(np.uint32)
    v, k = np.meshgrid(np.arange(n), np.arange(words), indexing="ij")
    fixed = (v + k) % 2 == 0
    w[fixed] = _PATTERNS[((v + 3 * k) // 2 % len(_PATTERNS))[fixed]]
    st = np.ascontiguousarray(w).reshape(-1).view(dt)
    assert st.shape == (n,)
    if m._prefix == "fm":
        st["modulator"]["reserved"] = 0
        st["carrier"]["reserved"] = 0
    if m._prefix == "curve_module" and n:
        st["current_song_note_offset"][0] = -1
        st["current_song_note_offset"][n - 1] = -(1 << 31)
    return st


def _same_bits(got, want, what):
    g, w = got.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)
    bad = np.nonzero(g != w)[0]
    words = max(1, got.dtype.itemsize // 4)
    assert bad.size == 0, f"{what}: {bad.size} words differ, the first at voice {bad[0] // words} word {bad[0] % words}: {g[bad[0]]:#010x} != {w[bad[0]]:#010x}"


def _round_trip(m, seed, what):
    st = _hostile(m, seed)
    m.set_state(st)
    _same_bits(m.state(), st, what)
    return st


# ------------------------------------------------------------------------------------------------ 1. init, round trip, NULL
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", NAMES)
def test_fresh_state_is_init_and_hostile_bits_round_trip(ctx, oracle, name, n):
    m = _make(name, n, ctx)
    st = m.state()
    assert st.shape == (n,)
    ref = _mods()[name][2]
    if ref is None:
        want = None
    else:
        o = getattr(oracle, ref[0])()
        getattr(oracle.lib(), ref[1])(C.byref(o), *ref[2])
        want = _leaves_ctypes(o)
        assert want == ([0.0, 1.0] if name == "decimator" else [0] * len(want)), (name, want)     # init(): zero, dcount = 1
    for v in range(n):
        got = _leaves_numpy(st[v])
        assert got == (want if want is not None else [0] * len(got)), (name, n, v, got)
    if name != "decimator":
        assert not st.tobytes().strip(b"\0"), (name, n)               # +0.0, not -0.0
    _round_trip(m, 7 * n + len(name), f"{name}, {n} voices: set_state -> state")
    _round_trip(m, 11 * n + len(name), f"{name}, {n} voices: a second set_state -> state")
    if name == "fm" and n:                                            # `reserved` is not state
        st = _hostile(m, 3)
        st["modulator"]["reserved"] = 0xFFFFFFFF
        st["carrier"]["reserved"] = 0x12345678
        m.set_state(st)
        st["modulator"]["reserved"] = 0
        st["carrier"]["reserved"] = 0
        _same_bits(m.state(), st, "fm: reserved reads 0")
    m.close()


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers_are_invalid(ctx, name):
    from zang_amd import abi
    lib = ctx.lib
    m = _make(name, 65, ctx)
    p = m._prefix
    extra = {"pmosc": (m._rel,) if name == "pmosc" else (), "fm": (C.c_uint32(1),)}.get(name, ())
    assert getattr(lib, f"zh_{p}_create")(ctx.handle, 65, *extra, None) == abi.ZH_ERR_INVALID
    h = C.c_void_p()
    assert getattr(lib, f"zh_{p}_create")(None, 65, *extra, C.byref(h)) == abi.ZH_ERR_INVALID
    st = m.state()
    assert getattr(lib, f"zh_{p}_get_state")(m.handle, None) == abi.ZH_ERR_INVALID
    assert getattr(lib, f"zh_{p}_set_state")(m.handle, None) == abi.ZH_ERR_INVALID
    assert getattr(lib, f"zh_{p}_get_state")(None, st.ctypes.data) == abi.ZH_ERR_INVALID
    assert getattr(lib, f"zh_{p}_set_state")(None, st.ctypes.data) == abi.ZH_ERR_INVALID
    assert getattr(lib, f"zh_{p}_destroy")(None) == abi.ZH_ERR_INVALID
    _same_bits(m.state(), st, f"{name}: the refused calls changed nothing")
    m.close()


# ------------------------------------------------------------------------------------------------ 2. the flipped buffer
def _inputs(ctx):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(99)
    v = np.arange(V)
    freq = (110.0 * 2.0 ** ((v % 37) / 12.0)).astype(np.float32)      # 110 .. 880 Hz
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(freq=dev(freq), color=dev((0.1 + 0.8 * (v % 11) / 11.0).astype(np.float32)), fake=dev(freq * np.float32(8.0)),
             dur=dev((0.002 + 0.03 * (v % 7) / 7.0).astype(np.float32)), rel=dev((0.1 + 0.4 * (v % 5) / 5.0).astype(np.float32)))
    d["fimg"] = ctx.image(F, V, fill=0.0)
    d["fimg"].copy_(d["freq"][None, :].expand(F, V) * (1.0 + 0.25 * torch.rand(F, 1, device="cuda", generator=g)))
    d["iimg"] = ctx.image(F, V, fill=0.0)
    d["iimg"].copy_(torch.rand(F, V, device="cuda", generator=g) * 2.0 - 1.0)
    return d


# name -> (dispatch row, the kernel only the range form launches, paint(m, span, out, first, zero_first, inputs))
def _flip_cases():
    from zang_amd import zang
    cub = zang.PaintCurve.cubed
    return {
        "sineosc": ("sine_ranges", "k_sineosc_ranges", lambda m, sp, o, first, zf, d:
                    m.paint(sp, [o], [], False, m.Params(SR, zang.constant(d["freq"]), zang.constant(0.0)), zero_first=zf)),
        "envelope": ("envelope_ranges", "k_envelope_ranges", lambda m, sp, o, first, zf, d:
                     m.paint(sp, [o], [], first, m.Params(SR, cub(0.004), cub(0.02), cub(0.03), 0.6, True), zero_first=zf)),
        "decimator": ("decimator_ranges", "k_decimator_ranges", lambda m, sp, o, first, zf, d:
                      m.paint(sp, [o], [], False, m.Params(SR, d["iimg"], d["fake"]), zero_first=zf)),
        "portamento": ("portamento_ranges", "k_portamento_ranges", lambda m, sp, o, first, zf, d:
                       m.paint(sp, [o], [], first, m.Params(SR, cub(d["dur"]), d["freq"], True, True), zero_first=zf)),
        "pmosc": ("pmosc_ranges", "k_pmosc_ranges", lambda m, sp, o, first, zf, d:
                  m.paint(sp, [o], None, first, m.Params(SR, d["freq"], True), zero_first=zf)),
        "pulseosc": ("pulse_ctrl_ranges", "k_pulseosc_ctrl_sums", lambda m, sp, o, first, zf, d:
                     m.paint(sp, [o], [], False, m.Params(SR, zang.buffer(d["fimg"]), d["color"]), zero_first=zf)),
    }


FLIP_NAMES = ["sineosc", "envelope", "decimator", "portamento", "pmosc", "pulseosc"]


@pytest.mark.parametrize("name", FLIP_NAMES)
def test_state_calls_address_the_flipped_buffer(ctx, name, monkeypatch):
    from zang_amd import modules as mod, zang
    _clear_env(monkeypatch)
    row, kernel, paint = _flip_cases()[name]
    util.set_form(monkeypatch, **{row: "2"})
    d = _inputs(ctx)
    make = (lambda: mod.PMOscInstrument(V, d["rel"], ctx)) if name == "pmosc" else (lambda: _make(name, V, ctx))
    whole, empty = zang.Span(0, F), zang.Span(F // 2, F // 2)

    m = make(); out = ctx.image(F, V, fill=0.5)
    paint(m, whole, out, True, True, d)
    ctx.sync()
    assert kernel in ctx.last_form(), (name, ctx.last_form())          # the form that writes the other buffer ran
    s1 = m.state()
    assert s1.tobytes().strip(b"\0"), name                             # the paint moved the state: the init buffer is not it
    hostile = _round_trip(m, 5, f"{name}: set_state -> state after a frame-range paint")
    if name == "pulseosc":                                             # no frame, no change, whatever the counter
        paint(m, empty, out, False, False, d)
        _same_bits(m.state(), hostile, "pulseosc: an empty span")
    m.set_state(s1)
    _same_bits(m.state(), s1, f"{name}: the paint's own state set again")
    paint(m, empty, out, False, False, d)
    _same_bits(m.state(), s1, f"{name}: an empty span, same params, no new note")
    paint(m, whole, out, False, False, d)
    ctx.sync()
    assert kernel in ctx.last_form(), (name, ctx.last_form())

    twice = make(); out2 = ctx.image(F, V, fill=0.5)                   # the same two paints, its state never read or set
    paint(twice, whole, out2, True, True, d)
    paint(twice, whole, out2, False, False, d)
    ctx.sync()
    util.assert_bitexact(out.cpu().numpy(), out2.cpu().numpy(), f"{name}: the image after set_state(the state read) and a second paint")
    _same_bits(m.state(), twice.state(), f"{name}: the state after both paints")
    m.close(); twice.close()
