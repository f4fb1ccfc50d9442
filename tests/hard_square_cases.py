"""The HardSquare voice tests' data, shared by tests/test_hard_square_reference.py and tests/test_gpu_hard_square.py; holds no
tests.  The tables, bases and hostile values are those of tests/lead_cases.py (ROWS 256, the span [3, 250), MAX_SPANS 4, the FIXED
shapes in voices 0-4); the reference is tests/arp_reference.py hard_square_paint under tests/lead_reference.py's Trigger loop."""
import numpy as np

from tests import arp_reference as ar
from tests import lead_cases as lc
from tests import lead_reference as lr

SR = lc.SR
VOICES = [1, 63, 64, 65, 200]
# Hostile values act from frame HOSTILE_FROM = 200 on: at most 50 of the 247 compared frames of a voice (0.2024) can turn NaN.  The
# cap sits above that share and far below 1, as lead_cases.NAN_CAP does; it is a condition on the INPUTS, checked on the oracle alone.
NAN_CAP = lc.NAN_CAP
assert (lc.SPAN[1] - lc.HOSTILE_FROM) / (lc.SPAN[1] - lc.SPAN[0]) < NAN_CAP


def voices(oracle, V):
    return [ar.HardSquareVoice(oracle) for _ in range(V)]


def reference_spans(oracle, vs, tb, img, sync, zero_first, sample_rate=SR, dflt=None, span=lc.SPAN):
    """the Trigger loop of every voice, in place on img and sync [V][ROWS]"""
    return lr.paint_spans(oracle, ar.hard_square_paint, vs, tb, img, sync, span, sample_rate, zero_first, None, dflt=dflt)


def reference_plain(oracle, vs, S, E, img, sync, sample_rate, freq, note_on):
    """Instrument.paint over [S, E) for every voice; freq and note_on scalars or per-voice arrays"""
    temps = [np.zeros(img.shape[1], np.float32) for _ in range(2)]
    at = lambda x, v: x[v] if isinstance(x, np.ndarray) else x
    for v in range(len(vs)):
        ar.hard_square_paint(oracle, vs[v], S, E, (img[v], None if sync is None else sync[v]), temps, False, sample_rate, at(freq, v),
                             bool(at(note_on, v)))


def cnts(vs):
    return np.array([v.cnt for v in vs], np.uint32)
