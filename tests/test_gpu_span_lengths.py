"""GPU: every exact paint of tests/paint_cases.py at the SPAN LENGTHS where its kernel form changes, against the oracle bit for bit.

The library picks a kernel form from the span's length as well as from the voice count:

    frames   what changes there
    1..9     the chunk loops: 8 frames plus a tail (seq.hip.h frame_loop), 4 or 3 frames (k_osc_const4)
    32       nothing, though modules.hip has a `>= 32` for the pink tap kernel: it never decides (see below)
    64       the wave pipelines (k_filter_pc, k_filter_pc_ctl, k_filtered_echoes_pc) and the delay's frames-at-once form
    128      the frame ranges (zh_range_frames, zh_noise_range_frames: with them k_noise_fix and the pink tap kernel), and
             k_noise_filter_ring
    136      a range of 8 frames leaves 17 ranges: a forced `*_ranges=64` is cut to what remains
    192      (delay_samples) a span longer than the delay is painted as successive pieces: below, at and past one length, past two
    2,048    the last length the white-noise ranges take: 32 ranges of 64 frames use table T^(32 * 62), the last but one

Every length `L` is painted in an image of L + 11 rows as the span (5, 5 + L): an odd start, rows above and below it.  V = 132 voices
(a multiple of 4, three waves, four live lanes in the last), every voice checked; carried paints, ZERO_FIRST then add; image columns
and final states bit for bit (paint_cases._check); canaries around everything -- a chunk loop that rounds a short span up writes
into the rows below it.  Form sets: `default`, `walks` (every row tests/test_gpu_views.py::_walk_rows names set to 0), `forced` (the
shapes only large voice counts reach: three ranges, 16-frame tiles, osc_fc = 3) and `forced64` (every `*_ranges` row 64: the cap,
and "at least two ranges remain").

test_the_form_flips_at_its_threshold asserts the kernels zh_last_form names on either side of a threshold: green bits at 128 frames
prove nothing if the range form was not taken.  One flip lies elsewhere than its own source line says: pink Noise takes k_pink_taps
only over white frame RANGES, so from 128 frames, not from the 32 of the tap kernel's own condition (which can never be false).

test_state_is_handed_from_one_form_to_the_next paints consecutive spans of different lengths with one module, so that a walk, a range
form, a single frame, a pipeline's tile pair, a 63-frame walk and a long range form follow each other on one state.
"""
import re

import numpy as np
import pytest

from tests import paint_cases as pc
from tests import util
from tests.test_gpu_dispatch import _table_rows
from tests.test_gpu_views import _clear_env, _walk_rows

pytestmark = pytest.mark.gpu
V = 132
LEAD, PAD = 5, 11                       # the span starts at row 5 of L + 11 rows
SHORT = [0, 1, 3, 4, 5, 7, 8, 9]
THRESHOLDS = [31, 32, 33, 63, 64, 65, 127, 128, 129, 136, 255, 256, 257]
DELAY, DELAY_LENGTHS = 192, [191, 192, 193, 385]      # 192: the least delay the role-wave echo form takes (delay.hip)
TALL = [2047, 2048, 2049, 4103]
PIECES = [(0, 127), (127, 255), (255, 256), (256, 320), (320, 383), (383, 1200)]
PIECE_CASES = ["sineosc_const", "sineosc_image", "pulse_const", "pulse_image", "trisaw_const", "trisaw_image", "decimator",
               "filter_lowpass_const", "filter_bandpass_const", "filter_notch_image", "filtered_echoes", "simple_delay", "cycle_const",
               "cycle_image", "noise_white", "noise_pink", "noise_filter_white", "envelope", "nice"]

RANGE_ROWS = sorted(n for n in _table_rows() if re.search(r"_ranges$", n))
WALK_ROWS = _walk_rows()
_FORCED = dict(pulse_ctrl_sums=0, trisaw_ctrl_quot=0, filter_pc_max=1, pink_taps=16, osc_fc=3)
FORM_SETS = {
    "default": {},
    "walks": {n: 0 for n in WALK_ROWS},
    "forced": dict({n: 3 for n in RANGE_ROWS}, **_FORCED),
    "forced64": dict({n: 64 for n in RANGE_ROWS}, **_FORCED),
}


def _set_forms(monkeypatch, forms):
    _clear_env(monkeypatch)
    if FORM_SETS[forms]:
        util.set_form(monkeypatch, **FORM_SETS[forms])


def _paint(ctx, oracle, L, names, geometry="plain", delay=300):
    """the cases `names` over the span (5, 5 + L) of L + 11 rows -> the Shared (its .forms: the kernels of each case's last paint)"""
    g = pc.Geometry(geometry, V, frames=L + PAD, span=(LEAD, LEAD + L), delay_samples=delay)
    sh = pc.Shared(ctx, V, np.arange(V, dtype=np.int64), g)
    g.check_canaries("the shared inputs")
    for name in names:
        pc.CASES[name](ctx, oracle, sh)                       # (each case ends with the canary check: Shared.finish)
    return sh


# ------------------------------------------------------------------------------------------------ 1. every case at every length
@pytest.mark.parametrize("geometry", ["plain", "shifted"])
@pytest.mark.parametrize("forms", ["default", "walks", "forced"])
def test_short_spans_equal_the_oracle(ctx, oracle, forms, geometry, monkeypatch):
    """0..9 frames: the chunk loops of 8, 4 and 3 frames and their tails.  An empty span changes nothing: not the image, not the
    guards (the window of the canary check is empty), not the state (the oracle's, after its own empty paints)."""
    _set_forms(monkeypatch, forms)
    for L in SHORT:
        _paint(ctx, oracle, L, list(pc.CASES), geometry)


@pytest.mark.parametrize("forms", list(FORM_SETS))
@pytest.mark.parametrize("L", THRESHOLDS)
def test_threshold_spans_equal_the_oracle(ctx, oracle, L, forms, monkeypatch):
    _set_forms(monkeypatch, forms)
    _paint(ctx, oracle, L, list(pc.CASES))


@pytest.mark.parametrize("forms", ["default", "walks", "forced"])
@pytest.mark.parametrize("L", DELAY_LENGTHS)
def test_spans_around_the_delay_length_equal_the_oracle(ctx, oracle, L, forms, monkeypatch):
    """a delay of 192 samples: a span below, at and past one delay length and past two -- the pieces of delay.hip, ring and index"""
    _set_forms(monkeypatch, forms)
    _paint(ctx, oracle, L, ["filtered_echoes", "simple_delay"], delay=DELAY)


@pytest.mark.parametrize("forms", ["default", "walks", "forced"])
@pytest.mark.parametrize("L", TALL)
def test_tall_spans_equal_the_oracle(ctx, oracle, L, forms, monkeypatch):
    """around 2,048 frames (the last length of the white-noise ranges: the tables T^(32 j) up to j = 62) and 4,103 (no multiple of
    8, more than 64 ranges of 64 frames, four tile quads of the pipelines and more)"""
    _set_forms(monkeypatch, forms)
    _paint(ctx, oracle, L, list(pc.CASES))


# ------------------------------------------------------------------------------------------------ 2. the form that ran
# (case, its name in Shared.forms, form set, kernel, the lengths without it, the lengths with it, the kernel that runs instead)
FLIPS = [
    ("envelope", "Envelope", "default", "k_envelope_ranges", [127], [128, 129], "k_envelope"),
    ("envelope", "Envelope", "forced", "k_envelope_ranges", [127], [128], "k_envelope"),
    ("sineosc_const", "SineOsc const", "default", "k_sineosc_ranges", [127], [128, 129], "k_sineosc"),
    ("sineosc_const", "SineOsc const", "forced64", "k_sineosc_ranges", [127], [128, 136], "k_sineosc"),
    ("filter_lowpass_const", "Filter type 1 const", "default", "k_filter_pc", [63], [64, 65], "k_filter"),
    # filter_pc_max = 1 < V: modules.hip launches k_filter_pc<., 16> (zh_last_form drops template arguments)
    ("filter_lowpass_const", "Filter type 1 const", "forced", "k_filter_pc", [63], [64, 65], "k_filter"),
    ("noise_white", "Noise white", "default", "k_noise_white_ranges", [127, 2049], [128, 2047, 2048], "k_noise"),
    ("noise_white", "Noise white", "default", "k_noise_fix", [127, 2049], [128, 2047, 2048], "k_noise"),
    ("noise_white", "Noise white", "forced", "k_noise_fix", [127, 2049], [128, 2048], "k_noise"),
    # the tap kernel's own condition is `end - start >= 32`, but it only ever follows white frame ranges: from 128 frames
    ("noise_pink", "Noise pink", "default", "k_pink_taps", [31, 32, 33, 127, 2049], [128, 2048], "k_noise"),
    ("noise_pink", "Noise pink", "forced", "k_pink_taps", [32, 127], [128], "k_noise"),
    ("noise_filter_white", "Noise->Filter fused, white", "default", "k_noise_filter_ring", [127], [128, 129], "k_noise_filter_pc"),
    ("simple_delay", "SimpleDelay", "default", "k_delay_frames", [63], [64, 65], "k_simple_delay"),
]


@pytest.mark.parametrize("k", range(len(FLIPS)), ids=[f"{f[0]}-{f[2]}-{f[3]}" for f in FLIPS])
def test_the_form_flips_at_its_threshold(ctx, oracle, k, monkeypatch):
    case, name, forms, kernel, without, with_, instead = FLIPS[k]
    _set_forms(monkeypatch, forms)
    ran = {L: _paint(ctx, oracle, L, [case]).forms[name] for L in without + with_}
    print(f"\n{case} [{forms}]: " + "; ".join(f"{L}: {','.join(ran[L])}" for L in sorted(ran)))
    for L in without:
        assert kernel not in ran[L] and instead in ran[L], (case, forms, L, ran[L])
    for L in with_:
        assert kernel in ran[L] and instead not in ran[L], (case, forms, L, ran[L])


# ------------------------------------------------------------------------------------------------ 3. state from form to form
@pytest.mark.parametrize("forms", ["default", "forced"])
@pytest.mark.parametrize("case", PIECE_CASES)
def test_state_is_handed_from_one_form_to_the_next(ctx, oracle, case, forms, monkeypatch):
    """1,200 rows painted as six consecutive spans by ONE module -- a 127-frame walk, 128 frames of ranges, one frame, a pipeline's
    tile pair (64), a 63-frame walk, an 817-frame range form -- the first with ZERO_FIRST, the rest adding; the oracle paints the
    same pieces.  What the reference's Trigger produces in every buffer: a note that starts near a buffer's end."""
    _set_forms(monkeypatch, forms)
    g = pc.Geometry("plain", V, frames=PIECES[-1][1], spans=PIECES)
    sh = pc.Shared(ctx, V, np.arange(V, dtype=np.int64), g)
    pc.CASES[case](ctx, oracle, sh)
