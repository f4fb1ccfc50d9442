"""GPU: every kernel form that is selected BY VOICE COUNT, against the ORACLE at the voice counts that select it.

The library picks a form per paint from the voice count (frame ranges with a state replay, wave pipelines with 32- or
16-frame tiles, one-wave walks ...; limits at 16,384 / 32,768 / 40,960 / 65,536 / 131,072 voices).  The small-voice-count
parity tests (test_gpu_modules.py ...) hold each form against the oracle where it can be forced through a switch; here every
module is painted in its DEFAULT form at each boundary voice count (and just past the last one) -- two carried buffers, the
first with ZERO_FIRST, the second adding -- and the image columns and final states of sampled voices (a stride through the
whole range, the first and the last voice, voices next to wave and block edges) are compared bit for bit with the oracle.
A second test forces the geometries that only large voice counts reach (2-3 white-noise ranges, 16-frame filter tiles,
2-4 Decimator / Curve / Envelope / ... ranges) at a small voice count, every voice checked.
"""
import ctypes as C

import numpy as np
import pytest

from tests import util
from tests.paint_cases import (CASES, Geometry, Shared, case_stateless,           # the cases: tests/paint_cases.py
                               sample_voices, _crafted_noise_state)                # noqa: F401  (names other tests import from here)

pytestmark = pytest.mark.gpu
SR = 48000.0
F = 1024
D = 300                 # delay samples of the echo modules


def _shared(ctx, V, idx):
    """the cases' inputs in the `plain` geometry: 1,024 rows, the whole image as the span, delays of 300 samples"""
    return Shared(ctx, V, idx, Geometry("plain", V, frames=F, span=(0, F), delay_samples=D))


# every limit a form is selected by (zh_range_frames callers, ZH_*_PC*_MAX defaults, noise_jump.hip), and just past the last
def _table_rows():
    """the library's dispatch table (csrc/dispatch.hip) through the C ABI: {name: default}; loads without a GPU"""
    from zang_amd import abi
    lib = abi.load()
    rows = {}
    for i in range(lib.zh_form_count()):
        name, doc, d, c = C.c_char_p(), C.c_char_p(), C.c_long(), C.c_long()
        assert lib.zh_form_info(i, C.byref(name), C.byref(d), C.byref(c), C.byref(doc)) == 0
        rows[name.value.decode()] = d.value
    return rows


def _boundary_voices():
    """Every voice-count threshold of the table (`*_max` / `*_min` rows between 16,384 and 131,072) and one wave past it, plus the
    voice limits of the frame-range forms (arguments of zh_range_frames at the call sites: 16,384 / 32,768 / 40,960 / 65,536 /
    131,072) and two counts between thresholds."""
    vs = set()
    for name, d in _table_rows().items():
        if (name.endswith("_max") or name.endswith("_min")) and 16384 <= d <= 131072:
            vs.update((d, d + 64))
    for d in (16384, 32768, 40960, 65536, 131072):
        vs.update((d, d + 64))
    vs.update((24576, 49152))
    return sorted(vs)


BOUNDARY_VOICES = _boundary_voices()


@pytest.mark.parametrize("V", BOUNDARY_VOICES)
def test_default_forms_equal_the_oracle_at_dispatch_boundaries(ctx, oracle, V, monkeypatch):
    import torch
    for name in list(__import__("os").environ):
        if name.startswith("ZH_") and name not in ("ZH_ENV_LIVE",):
            monkeypatch.delenv(name)                           # default dispatch, whatever the suite was started with
    idx = sample_voices(V)
    sh = _shared(ctx, V, idx)
    for name, case in CASES.items():
        case(ctx, oracle, sh)
        torch.cuda.empty_cache()


FORCED = [
    # (switches, cases they matter for): geometries that only large voice counts reach, at 333 voices, every voice checked
    ({"noise_ranges": "2"}, ["noise_white", "noise_white_add", "noise_pink"]),
    ({"noise_ranges": "3"}, ["noise_white", "noise_white_add", "noise_pink"]),
    ({"noise_ranges": "0"}, ["noise_white", "noise_pink", "noise_filter_white"]),
    ({"pink_taps": "16", "noise_ranges": "2"}, ["noise_pink"]),
    ({"filter_pc_max": "1"}, ["filter_lowpass_const", "filter_bandpass_const"]),           # 16-frame tiles (ZH_FILTER_PC16_MAX default)
    ({"filter_pc_max": "0"}, ["filter_lowpass_const", "filter_bandpass_const"]),           # the one-wave walk
    ({"decimator_ranges": "2"}, ["decimator"]), ({"decimator_ranges": "3"}, ["decimator"]),
    ({"curve_ranges": "2"}, ["curve_linear", "curve_smoothstep"]), ({"curve_ranges": "3"}, ["curve_linear", "curve_smoothstep"]),
    ({"envelope_ranges": "2"}, ["envelope"]), ({"envelope_ranges": "3"}, ["envelope"]),
    ({"portamento_ranges": "2"}, ["portamento"]), ({"portamento_ranges": "5"}, ["portamento"]),
    ({"cycle_ranges": "2"}, ["cycle_const"]), ({"cycle_ranges": "3"}, ["cycle_const", "cycle_image"]),
    ({"sine_ranges": "2"}, ["sineosc_const", "sineosc_image"]), ({"sine_ranges": "3"}, ["sineosc_const", "sineosc_image"]),
    ({"sampler_ranges": "2"}, ["sampler"]), ({"sampler_ranges": "3"}, ["sampler"]),
    ({"pulse_ctrl_ranges": "2"}, ["pulse_image"]), ({"pulse_ctrl_ranges": "3", "pulse_ctrl_sums": "0"}, ["pulse_image"]),
    ({"trisaw_ctrl_ranges": "2"}, ["trisaw_image"]), ({"trisaw_ctrl_ranges": "3", "trisaw_ctrl_quot": "0"}, ["trisaw_image"]),
    ({"pmosc_ranges": "2"}, ["pmosc"]), ({"pmosc_ranges": "3"}, ["pmosc"]),
    ({"nice_pc4_max": "0"}, ["nice"]), ({"nice_pc_max": "0"}, ["nice"]),
    ({"nf_ring_max": "0"}, ["noise_filter_white"]), ({"nf_ring_max": "0", "nf_pc_max": "0"}, ["noise_filter_white", "noise_filter_pink"]),
    ({"echoes_pc_max": "0"}, ["filtered_echoes"]), ({"delay_frames_max": "0"}, ["simple_delay"]),
]


@pytest.mark.parametrize("k", range(len(FORCED)))
def test_forced_large_voice_count_geometries_at_a_small_voice_count(ctx, oracle, k, monkeypatch):
    env, names = FORCED[k]
    for name in list(__import__("os").environ):
        if name.startswith("ZH_") and name not in ("ZH_ENV_LIVE",):
            monkeypatch.delenv(name)
    for n, v in env.items():
        util.set_form(monkeypatch, **{n: v})
    V = 333
    sh = _shared(ctx, V, np.arange(V, dtype=np.int64))
    for name in names:
        CASES[name](ctx, oracle, sh)


@pytest.mark.parametrize("V", [1280, 4100])
def test_distortion_chunked_form_forced_at_a_small_voice_count(ctx, oracle, V, monkeypatch):
    """k_distortion_chunks (four voices per lane, the per-voice constants once per workgroup through LDS; default from
    distortion_rows_min voices) forced at voice counts whose last workgroup is partial: both types, `+=` after ZERO_FIRST, every voice
    against the oracle bit for bit; the kernel that ran is checked."""
    for name in list(__import__("os").environ):
        if name.startswith("ZH_") and name not in ("ZH_ENV_LIVE",):
            monkeypatch.delenv(name)
    util.set_form(monkeypatch, distortion_rows_min=0)
    sh = _shared(ctx, V, np.arange(V, dtype=np.int64))
    case_stateless(ctx, oracle, sh)
    assert ctx.last_form() == ["k_distortion_chunks"], ctx.last_form()
    util.set_form(monkeypatch, distortion_rows_min=1 << 30)
    case_stateless(ctx, oracle, sh)
    assert ctx.last_form() == ["k_distortion"], ctx.last_form()
