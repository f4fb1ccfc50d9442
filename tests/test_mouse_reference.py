"""CPU: the yardstick of the controlled phase-modulation voice (tests/mouse_reference.py) against what is already pinned and
against itself.  With constant ratio = multiplier = 1.0, relative on and the patch's release it is the oracle's PMOscInstrument
(zo_pmosc_paint, examples/modules.zig:80-128) bit for bit; the carried temp shows exactly on the stream the cases file names;
the three-cursor model cuts every stream as the span walk does; MainModule follows the example's key and mouse rules."""
import ctypes as C

import numpy as np

from tests import mouse_cases as mc
from tests import mouse_reference as mr

f32 = np.float32


def test_constants_of_one_are_the_pinned_pmosc_instrument(oracle):
    L = oracle.lib()
    patch = mr.Patch(release=0.004, attack=0.025, decay=0.1, sustain_volume=0.5)       # zo_pmosc's attack, decay and sustain
    ref = oracle.PMOscInstrument()
    L.zo_pmosc_init(C.byref(ref), 0.004)
    voice = mr.Voice(oracle)
    out_a, out_b = np.zeros(96, f32), np.zeros(96, f32)
    ta, tb = [np.zeros(96, f32) for _ in range(3)], [np.zeros(96, f32) for _ in range(3)]
    for s, e, nic, freq, on in [(0, 30, 1, 220.0, 1), (30, 31, 0, 330.0, 1), (31, 70, 0, 330.0, 0), (70, 96, 1, 110.0, 1)]:
        L.zo_pmosc_paint(C.byref(ref), s, e, oracle.fptr(out_a), *(oracle.fptr(t) for t in ta), nic, mc.SR, freq, on)
        mr.instr_paint(oracle, voice, s, e, out_b, tb, nic, mc.SR, freq, on, True, ("c", 1.0), ("c", 1.0), patch)
    assert np.array_equal(out_a.view(np.uint32), out_b.view(np.uint32)) and float(np.abs(out_a).max()) > 0.05
    assert (voice.carrier.t, voice.modulator.t, voice.env.state) == (ref.carrier.t, ref.modulator.t, ref.env.state)


def _two_buffers(oracle, V, carried, relative):
    voices = [mr.Voice(oracle) for _ in range(V)]
    stale = np.zeros((V, mc.ROWS), f32) if carried else None
    outs = []
    for b in range(2):
        img = np.zeros((V, mc.ROWS), f32)
        mr.paint_controlled(oracle, voices, mc.held_note(V, b), img, stale, mc.SPANS[96], mc.SR, True, relative, mc.SCALES[relative], mc.PATCH)
        outs.append(img)
    return outs, stale


def test_the_carried_temp_shows_on_the_held_note_in_relative_mode_only(oracle):
    (a0, a1), stale = _two_buffers(oracle, 2, True, True)
    (z0, z1), _ = _two_buffers(oracle, 2, False, True)
    S, E = mc.SPANS[96]
    assert np.array_equal(a0.view(np.uint32), z0.view(np.uint32))      # the first buffer reads a row of zeros either way
    assert not np.array_equal(a1[:, S:E].view(np.uint32), z1[:, S:E].view(np.uint32))
    assert float(stale[:, S:E].min()) > 0.0 and np.all(stale[:, :S] == 0.0)            # the image holds the (held) envelope
    (a0, a1), _ = _two_buffers(oracle, 2, True, False)
    (z0, z1), _ = _two_buffers(oracle, 2, False, False)
    assert np.array_equal(a1.view(np.uint32), z1.view(np.uint32))      # the absolute branch is a copy: s is never read


def test_each_stream_is_cut_as_the_span_walk_cuts_it():
    for seed in range(8):
        tables = mc.streams(16, 96, seed)
        for v in range(16):
            ev = mr.segments(tables, v, *mc.SPANS[96])
            for s in range(3):
                begun = [e[2] for e in ev if e[0] == "begin" and e[1] == s]
                assert begun == [k for k, _, _ in mr.walk(tables[s], v, *mc.SPANS[96])]
                covered = sorted(f for e in ev if e[0] == "seg" and e[3] >> s & 1 for f in range(e[1], e[2]))
                assert covered == sorted(f for _, a, b in mr.walk(tables[s], v, *mc.SPANS[96]) for f in range(a, b))
            segs = [e for e in ev if e[0] == "seg"]
            assert segs[0][1] == mc.SPANS[96][0] and segs[-1][2] == mc.SPANS[96][1] and all(a[2] == b[1] for a, b in zip(segs, segs[1:]))


def test_main_module_follows_the_examples_events(oracle):
    m = mr.MainModule(oracle, sample_rate=mc.SR, patch=mc.PATCH)
    assert m.key(7, False, 1.0, 0) is None                             # a release of a key that is not held
    m.mouse(0.5, 0.25, 3)
    assert m.key(7, True, 1.5, 10) == (f32(660.0), True)
    quiet_then_note = m.paint(64)
    assert not quiet_then_note[:10].any() and float(np.abs(quiet_then_note[10:]).max()) > 0.01
    assert m.key(8, False, 2.0, 0) is None and m.keys.held == 7        # ... still not the held one
    m.space()
    assert m.keys.mode == 1
    assert m.key(7, False, 1.5, 5) == (f32(660.0), False) and m.keys.held is None
    released = m.paint(64)
    assert float(np.abs(released[:5]).max()) > 0.01
    assert m.voice.env.state in (0, 4)                                 # releasing, or done
