"""GPU: every paint against the ORACLE with non-finite, zero, negative, denormal, huge and threshold values in its parameter
slots and carried state words -- the table of tests/hostile_cases.py (one slot of the ordinary tuple at a time, a few interacting
pairs; every hostile voice once alone among the ordinary voices of its wave or 256-voice group and once among hostile voices
only), in every kernel form a switch selects.

The contract (include/zang_hip.h): the device does what the reference does for ANY f32, and what the oracle
defines where the reference asserts.  The fast forms decide by wave votes over compares that a NaN fails (EnvLaneT::quiet,
SineOscLane::small_args, k_osc_const4's "no silent voice", trisaw_all_saw ...): one hostile voice changes the path of its 63 or
255 neighbours, and a wrong sense of one NaN compare shows only here.

Compared: NaN positions equal; every other sample and float state word bit for bit (the signs of zeros and infinities included);
integer state equal outright; a NaN's sign and payload are not compared.  tests/test_cpp_hostile_oracle.py shows on the CPU that
the oracle is defined on the whole table and that at most half of the hostile voices' reference samples are NaN.
"""
import os

import numpy as np
import pytest

from tests import hostile_cases as hc
from tests import util

pytestmark = pytest.mark.gpu

# the one-wave forms: the row set of tests/test_gpu_fuzz.py::test_fuzz_again_with_the_single_wave_forms
ONE_WAVE = dict(nice_pc_max=0, nf_pc_max=0, nf_ring_max=0, noise_ranges=0, sine_ranges=0, sampler_ranges=0, pink_taps=0, decimator_ranges=0,
                envelope_ranges=0, portamento_ranges=0, pulse_ctrl_ranges=0, trisaw_ctrl_ranges=0, pink_pipe_max=0, filter_pc_max=0, echoes_pc_max=0)

# module -> the cases of tests/paint_cases.py whose forced geometries (tests/test_gpu_dispatch.py::FORCED) apply to it
FORCED_CASES = {"SineOsc": {"sineosc_const", "sineosc_image"}, "PulseOsc": {"pulse_image"}, "TriSawOsc": {"trisaw_image"},
                "Cycle": {"cycle_const", "cycle_image"}, "Envelope": {"envelope"}, "Portamento": {"portamento"}, "Decimator": {"decimator"},
                "Filter": {"filter_lowpass_const", "filter_bandpass_const", "filter_notch_image"}, "Distortion": set(),
                "NiceInstrument": {"nice"}, "PMOscInstrument": {"pmosc"}, "FilteredEchoes": {"filtered_echoes"},
                "Curve": {"curve_linear", "curve_smoothstep"}, "Gate": set(), "Sampler": {"sampler"},
                "NoiseFilter": {"noise_filter_white", "noise_filter_pink"}, "FilteredSawtooth": set(), "HardSquare": set(), "StereoEchoes": set()}


def _forced(name):
    from tests.test_gpu_dispatch import FORCED
    return [env for env, cases in FORCED if FORCED_CASES[name] & set(cases)]


def _forms(name):
    """[(id, dispatch rows, keyword arguments of _run)]"""
    out = [("default", {}, {}), ("walks", "walks", {}), ("one_wave", ONE_WAVE, {})]
    out += [("forced-" + "-".join(f"{k}={v}" for k, v in env.items()), env, {}) for env in _forced(name)]
    if name in ("PulseOsc", "TriSawOsc"):
        out += [("const4-params_unchanged", {}, dict(unchanged=True)), ("const-1022", {}, dict(n_voices=1022)),
                ("paint_batch", {}, dict(batch=True)), ("paint_batch-params_unchanged", {}, dict(batch=True, unchanged=True))]
    if name == "Distortion":
        out += [("chunks", dict(distortion_rows_min=0), {}), ("rows", dict(distortion_rows_min=1 << 30), {})]
    if name in ("FilteredSawtooth", "HardSquare"):      # the generated kernel's three forms (the default above: the library's choice)
        out += [("lane", dict(script_pc=0, script_ranges=0), {}), ("script_ranges", dict(script_pc=0, script_ranges=3), {}),
                ("role_waves", dict(script_pc=1), dict(roles=True))]
    return out


CASES = [(name, fid) for name in hc.MODULES for fid, _, _ in _forms(name)]

# The kernels a form must (and must not) have launched, where a switch or the voice count selects the form: (module, form id) ->
# [(part of the variant's label, kernels that ran in some paint of it, kernels that ran in none)], over zh_last_form of every paint.
# (Filter's bypass is a plain add, k_elementwise, in every form.)
def _ranges(base, rows):
    """a module whose frame-range form is k_<base>_ranges: default and forced take it, the walks and one-wave forms never do"""
    out = {"default": [("", {base + "_ranges"}, set())], "walks": [("", {base}, {base + "_ranges"})], "one_wave": [("", {base}, {base + "_ranges"})]}
    out.update({"forced-" + r: [("", {base + "_ranges"}, set())] for r in rows})
    return out


EXPECT = {
    "SineOsc": _ranges("k_sineosc", ["sine_ranges=2", "sine_ranges=3"]),
    "Envelope": _ranges("k_envelope", ["envelope_ranges=2", "envelope_ranges=3"]),
    "Portamento": _ranges("k_portamento", ["portamento_ranges=2", "portamento_ranges=5"]),
    "Decimator": _ranges("k_decimator", ["decimator_ranges=2", "decimator_ranges=3"]),
    "PulseOsc": {
        "default": [("constant", {"k_osc_const4"}, {"k_osc_const"}), ("freq image", {"k_pulseosc_ctrl", "k_pulseosc_ctrl_sums"}, set())],
        "walks": [("freq image", {"k_pulseosc_ctrl"}, {"k_pulseosc_ctrl_sums"})],
        "one_wave": [("freq image", {"k_pulseosc_ctrl"}, {"k_pulseosc_ctrl_sums"})],
        "forced-pulse_ctrl_ranges=2": [("freq image", {"k_pulseosc_ctrl", "k_pulseosc_ctrl_sums"}, set())],
        "forced-pulse_ctrl_ranges=3-pulse_ctrl_sums=0": [("freq image", {"k_pulseosc_ctrl"}, {"k_pulseosc_ctrl_sums"})],
        "const4-params_unchanged": [("constant", {"k_osc_const4"}, {"k_osc_const"})],
        "const-1022": [("constant", {"k_osc_const"}, {"k_osc_const4"})],
        "paint_batch": [("constant", {"k_osc_const4"}, {"k_osc_const"})], "paint_batch-params_unchanged": [("constant", {"k_osc_const4"}, {"k_osc_const"})],
    },
    "TriSawOsc": {
        "default": [("constant", {"k_osc_const4"}, {"k_osc_const"}), ("freq image", {"k_trisawosc_ctrl", "k_div_image"}, set())],
        "walks": [("freq image", {"k_trisawosc_ctrl"}, {"k_div_image"})],
        "one_wave": [("freq image", {"k_trisawosc_ctrl"}, {"k_div_image"})],
        "forced-trisaw_ctrl_ranges=2": [("freq image", {"k_trisawosc_ctrl", "k_div_image"}, set())],
        "forced-trisaw_ctrl_ranges=3-trisaw_ctrl_quot=0": [("freq image", {"k_trisawosc_ctrl"}, {"k_div_image"})],
        "const4-params_unchanged": [("constant", {"k_osc_const4"}, {"k_osc_const"})],
        "const-1022": [("constant", {"k_osc_const"}, {"k_osc_const4"})],
        "paint_batch": [("constant", {"k_osc_const4"}, {"k_osc_const"})], "paint_batch-params_unchanged": [("constant", {"k_osc_const4"}, {"k_osc_const"})],
    },
    # Cycle's and Curve's frame ranges are k_cycle / k_curve with more rows of blocks: one kernel name in every form
    "Cycle": {f: [("", {"k_cycle"}, set())] for f in ("default", "walks", "one_wave", "forced-cycle_ranges=2", "forced-cycle_ranges=3")},
    "Curve": {f: [("", {"k_curve"}, set())] for f in ("default", "walks", "one_wave", "forced-curve_ranges=2", "forced-curve_ranges=3")},
    "Sampler": {f: [("", {"k_sampler"}, set())] for f in ("default", "walks", "one_wave", "forced-sampler_ranges=2", "forced-sampler_ranges=3")},
    "NoiseFilter": {
        "default": [("white", {"k_noise_filter_ring"}, {"k_noise_filter"}), ("pink", {"k_noise_filter_pc"}, {"k_noise_filter"})],
        "forced-nf_ring_max=0": [("", {"k_noise_filter_pc"}, {"k_noise_filter_ring", "k_noise_filter"})],
        "forced-nf_ring_max=0-nf_pc_max=0": [("", {"k_noise_filter"}, {"k_noise_filter_ring", "k_noise_filter_pc"})],
        "walks": [("", {"k_noise_filter"}, {"k_noise_filter_ring", "k_noise_filter_pc"})],
        "one_wave": [("", {"k_noise_filter"}, {"k_noise_filter_ring", "k_noise_filter_pc"})],
    },
    "FilteredSawtooth": {
        "lane": [("constant", set(), {"zs_paint_pc_FilteredSawtooth"}), ("freq image", set(), {"zs_paint_pc_FilteredSawtoothCtl"})],
        "script_ranges": [("constant", set(), {"zs_paint_pc_FilteredSawtooth"}), ("freq image", set(), {"zs_paint_pc_FilteredSawtoothCtl"})],
        "role_waves": [("constant", {"zs_paint_pc_FilteredSawtooth"}, set()), ("freq image", {"zs_paint_pc_FilteredSawtoothCtl"}, set())],
    },
    "StereoEchoes": {"default": [("", {"k_stereo_echoes_pc"}, {"k_stereo_echoes"})], "walks": [("", {"k_stereo_echoes"}, {"k_stereo_echoes_pc"})],
                     "one_wave": [("", {"k_stereo_echoes_pc"}, set())]},     # (stereo_echoes_pc_max is not among the one-wave rows)
    "HardSquare": {
        "lane": [("", set(), {"zs_paint_pc_HardSquare"})], "script_ranges": [("", set(), {"zs_paint_pc_HardSquare"})],
        "role_waves": [("", {"zs_paint_pc_HardSquare"}, set())],
    },
    "Distortion": {
        "default": [("", {"k_distortion"}, {"k_distortion_chunks"})], "rows": [("", {"k_distortion"}, {"k_distortion_chunks"})],
        "chunks": [("", {"k_distortion_chunks"}, {"k_distortion"})],
    },
    "NiceInstrument": {
        "default": [("", {"k_nice_pc4"}, {"k_nice_pc"})], "forced-nice_pc4_max=0": [("", {"k_nice_pc"}, {"k_nice_pc4"})],
        "forced-nice_pc_max=0": [("", {"k_nice"}, {"k_nice_pc", "k_nice_pc4"})], "walks": [("", {"k_nice"}, {"k_nice_pc", "k_nice_pc4"})],
        "one_wave": [("", {"k_nice"}, {"k_nice_pc", "k_nice_pc4"})],
    },
    "PMOscInstrument": {
        "default": [("", {"k_pmosc_ranges"}, set())], "walks": [("", {"k_pmosc"}, {"k_pmosc_ranges"})],
        "forced-pmosc_ranges=2": [("", {"k_pmosc_ranges"}, set())], "forced-pmosc_ranges=3": [("", {"k_pmosc_ranges"}, set())],
        "one_wave": [("", {"k_pmosc_ranges"}, set())],                  # (pmosc_ranges is not among the one-wave rows)
    },
    "FilteredEchoes": {
        "default": [("", {"k_filtered_echoes_pc"}, set())], "walks": [("", {"k_filtered_echoes"}, {"k_filtered_echoes_pc"})],
        "one_wave": [("", {"k_filtered_echoes"}, {"k_filtered_echoes_pc"})],
        "forced-echoes_pc_max=0": [("", {"k_filtered_echoes"}, {"k_filtered_echoes_pc"})],
    },
    "Filter": {
        "default": [(", constant", {"k_filter_pc"}, {"k_filter"}), (", cutoff and resonance images", {"k_filter_pc_ctl"}, {"k_filter"})],
        "walks": [("", {"k_filter"}, {"k_filter_pc", "k_filter_pc_ctl"})],
        # (filter_pc_ctl_max, the row of the control-image pipeline, is in none of these three row sets)
        "one_wave": [(", constant", {"k_filter"}, {"k_filter_pc"}), (", cutoff and resonance images", {"k_filter_pc_ctl"}, {"k_filter"})],
        "forced-filter_pc_max=1": [(", constant", {"k_filter_pc"}, {"k_filter"}), (", cutoff and resonance images", {"k_filter_pc_ctl"}, {"k_filter"})],
        "forced-filter_pc_max=0": [(", constant", {"k_filter"}, {"k_filter_pc"}), (", cutoff and resonance images", {"k_filter_pc_ctl"}, {"k_filter"})],
    },
}

def _report(what, voices, hostile, nans, samples):
    """what a test compared, on its output (pytest -s / -rP shows it): voices, hostile voices, the oracle's NaN share among the latter"""
    print(f"{what}: {voices} voices compared, {hostile} hostile, NaN share {nans / max(samples, 1):.4f}")


def _set_rows(monkeypatch, rows):
    for n in list(os.environ):
        if n.startswith("ZH_") and n != "ZH_ENV_LIVE":
            monkeypatch.delenv(n)                                   # default dispatch, whatever the suite was started with
    if rows == "walks":
        from tests.test_gpu_views import WALK_ROWS
        rows = {n: 0 for n in WALK_ROWS}
    if rows:
        util.set_form(monkeypatch, **rows)


def _run(ctx, oracle, name, fid, n_voices=hc.V, unchanged=False, batch=False, roles=False):
    mod = hc.module(name)
    voices = hostile = nans = samples = 0
    seen = {}
    for va in mod.variants():
        for c, recs in enumerate(mod.chunks(va, n_voices)):
            got, words, extra, forms = hc.paint_device(ctx, mod, va, recs, unchanged=unchanged, batch=batch, oracle=oracle, roles=roles)
            a, b, x, y = hc.compare_chunk(oracle, mod, va, recs, got, words, extra, f"{name}, {fid}, chunk {c}", batch=batch)
            voices += a; hostile += b; nans += x; samples += y
            seen.setdefault(va.label, set()).update(k for f in forms for k in f)
    _report(f"{name}, {fid}", voices, hostile, nans, samples)
    return seen


def _check_kernels(name, fid, seen):
    for part, ran, never in EXPECT.get(name, {}).get(fid, []):
        for label, kernels in seen.items():
            if part in label and "hostile sample rate" not in label and "bypass" not in label:
                assert ran <= kernels and not (never & kernels), (name, fid, label, sorted(kernels), sorted(ran), sorted(never))


@pytest.mark.parametrize("name,fid", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_hostile_parameters_equal_the_oracle(ctx, oracle, name, fid, monkeypatch):
    rows, kw = next((r, k) for f, r, k in _forms(name) if f == fid)
    _set_rows(monkeypatch, rows)
    _check_kernels(name, fid, _run(ctx, oracle, name, fid, **kw))


# ------------------------------------------------------------------------------------------------ the sub-span forms
# k_<module>_spans: the hostile values in the per-sub-span `f` arrays, for the cases of tests/module_spans_cases.py.  Eight of its ten
# modules run: Noise and Gate have no float field.  (The Sampler's rate reaches an address; why no rate can take a load out of the
# sample is argued in tests/test_sample_kit_host.py.)  Three sub-spans per voice, their boundaries differing by voice; a hostile value
# stands in ONE sub-span of its voice, so the state it leaves is carried into an ordinary one.  Two buffers, the first ZERO_FIRST
# over garbage, the second adding.
SPAN_CASES = ["sineosc", "pulseosc", "trisawosc", "envelope", "filter", "decimator", "distortion", "sampler"]


def _sub_spans(V):
    v = np.arange(V)
    e0 = 100 + v % 11
    s1 = e0 + np.where(v % 4 == 0, 0, v % 5)
    e1 = 220 + v % 13
    start = np.stack([13 + v % 7, s1, e1 + v % 3]).astype(np.uint32)
    end = np.stack([e0, e1, 334 + v % 19]).astype(np.uint32)
    nic = np.stack([(v + k) % 2 for k in range(3)]).astype(np.uint8)
    return np.full(V, 3, np.uint32), start, end, nic


@pytest.mark.parametrize("name", SPAN_CASES)
def test_hostile_values_in_span_arrays_equal_the_oracle(ctx, oracle, name, monkeypatch):
    from tests import module_spans_cases as msc
    from zang_amd import zang
    _set_rows(monkeypatch, {})
    V, F, K = hc.V, hc.F, 3
    L = oracle.lib()
    case = msc.CASES[name]()
    rng = np.random.default_rng(31)
    floats = [n for n, gen in case.fields if gen(rng, (1,))[0] is not None]
    hv = [(n, x) for n in floats for x in hc.HOSTILE]
    count, start, end, nic = _sub_spans(V)
    assert int(end.max()) <= F
    per_run, compared, nans, samples = 14, 0, 0, 0
    for run in range((len(hv) + per_run - 1) // per_run):
        m = case.make(ctx, V)
        sts = [case.oracle_init(oracle, L) for _ in range(V)]
        case.dflt = msc._defaults(case, rng, V)
        case.arr = {n: gen(rng, (K, V)) for n, gen in case.fields}
        hostile = {}
        for j, (n, x) in enumerate(hv[run * per_run:(run + 1) * per_run]):          # alone in waves 1..14
            v = (1 + j) * 64 + (37 * (run * per_run + j) + 5) % 64
            case.arr[n][0][(run + j) % K, v] = x; hostile[v] = (n, x)
        for j in range(64):                                                          # wave 15: hostile voices only
            n, x = hv[(run * 64 + j) % len(hv)]
            case.arr[n][0][j % K, 15 * 64 + j] = x; hostile[15 * 64 + j] = (n, x)
        ex, extra = {}, {}
        if case.inputs:
            ex["input_host"] = rng.uniform(-1, 1, (V, F)).astype(np.float32)
            extra["input"] = util.to_image(ex["input_host"])
        ref = rng.uniform(-2, 2, (V, F)).astype(np.float32)
        out = util.to_image(ref)
        table = m.span_table(count, start, end, nic, case.arr)
        for b in range(2):
            if b == 0:
                ref[:, 13:F] = 0.0
            for v in range(V):
                for k in range(K):
                    case.oracle_paint(oracle, L, sts[v], v, int(start[k, v]), int(end[k, v]), ref[v], int(nic[k, v]), k, ex)
            m.paint_spans(zang.Span(13, F), [out], None, case.params(m, case.dflt, extra), table, zero_first=b == 0)
            ctx.sync()
            assert ctx.last_form() == ["k_%s_spans" % case.name], ctx.last_form()
            d = hc.first_difference(util.from_image(out), ref)
            if d is not None:
                (v, f), g, w, nbad = d
                raise AssertionError(f"{name} spans, run {run} buffer {b}: {nbad} samples differ, first at voice {v} (hostile: {hostile.get(v)}; sub-spans "
                                     f"{[(int(start[k, v]), int(end[k, v])) for k in range(K)]}) frame {f}: device {g!r}, oracle {w!r}")
            for gpu, cpu in case.state(m, sts):
                if gpu.dtype == np.float32:
                    assert hc.same_f32(gpu, cpu), (name, run, b, hc.first_difference(gpu, cpu))
                else:
                    assert np.array_equal(gpu, cpu), (name, run, b)
        hs = sorted(hostile)
        compared += len(hs); nans += int(np.isnan(ref[hs]).sum()); samples += ref[hs].size
        m.close()
    assert nans <= samples // 2, (name, nans, samples)               # the comparison is not hollow: at most half NaN
    _report(f"{name}, k_{name}_spans", V * ((len(hv) + per_run - 1) // per_run), compared, nans, samples)


# ------------------------------------------------------------------------------------------------ the instruments' span tables
# zh_nice_paint_spans / zh_pmosc_paint_spans: a hostile frequency in ONE sub-span of a voice's table, a hostile colour / release
# duration, or a hostile carried envelope painter.  1,024 voices take the lane-per-voice walk (k_*_spans), 64 the wave-per-voice
# form (k_*_spans_wave: the envelope's clock through EnvLane::block64, its stage end by a ballot over `t >= 1`), where the sample
# rate is hostile too in further runs.
def _instrument_items():
    items = [("freq", x) for x in hc.with_thresholds(hc.SR / 8, 0.0)] + [("own", x) for x in hc.HOSTILE]
    for x in hc._PAINTER:
        items += [("env.t", x), ("env.last_value", x), ("env.start", x)]
    return items


@pytest.mark.parametrize("V", [1024, 64])
@pytest.mark.parametrize("name", ["nice", "pmosc"])
def test_hostile_values_in_instrument_span_tables_equal_the_oracle(ctx, oracle, name, V, monkeypatch):
    import ctypes as C
    from zang_amd import modules as mod, zang
    from zang_amd.spans import SpanTable
    _set_rows(monkeypatch, {})
    F, K = hc.F, 3
    L = oracle.lib()
    desc = hc.module("NiceInstrument" if name == "nice" else "PMOscInstrument")
    items = _instrument_items()
    count, start, end, nic = _sub_spans(V)
    v_ = np.arange(V)
    on = np.stack([(v_ + k) % 3 != 0 for k in range(K)]).astype(np.uint8)
    per_run = 14 if V > 64 else 51
    rates = [hc.SR] if V > 64 else [hc.SR, np.nan, -1.0, np.inf]
    t0, t1, t2 = (np.zeros(F, np.float32) for _ in range(3))
    compared = nans = samples = 0
    for sr in rates:
        for run in range((len(items) + per_run - 1) // per_run):
            freq = np.tile(desc.freq[:V], (K, 1)).astype(np.float32)
            own = np.array([desc.ordinary(v)[1] for v in range(V)], np.float32)
            env = {}                                                        # voice -> (state, t, last_value, start)
            where = {}
            chosen = list(enumerate(items[run * per_run:(run + 1) * per_run]))
            places = [((1 + j) * 64 + (37 * (run * per_run + j) + 5) % 64, it) for j, it in chosen] if V > 64 else [(13 + j, it) for j, it in chosen]
            if V > 64:
                places += [(15 * 64 + j, items[(run * 64 + j) % len(items)]) for j in range(64)]
            for v, (slot, x) in places:
                where[v] = (slot, x)
                if slot == "freq":
                    freq[(run + v) % K, v] = x
                elif slot == "own":
                    own[v] = x
                else:
                    w = [1 + v % 4, np.float32(0.4), np.float32(0.3), np.float32(0.1)]
                    w[1 + ("env.t", "env.last_value", "env.start").index(slot)] = x
                    env[v] = w
            sts = []
            for v in range(V):
                if name == "nice":
                    s = oracle.NiceInstrument(); L.zo_nice_init(C.byref(s), float(own[v]))
                else:
                    s = oracle.PMOscInstrument(); L.zo_pmosc_init(C.byref(s), float(own[v]))
                if v in env:
                    s.env.state, s.env.painter.t, s.env.painter.last_value, s.env.painter.start = env[v]
                sts.append(s)
            m = (mod.NiceInstrument if name == "nice" else mod.PMOscInstrument)(V, util.dev(own), ctx)
            if env:
                st = m.state()
                for v, w in env.items():
                    st["env"]["state"][v], st["env"]["t"][v], st["env"]["last_value"][v], st["env"]["start"][v] = w
                m.set_state(st)
            table = SpanTable.from_arrays(count, start, end, freq, on, nic, ctx.device)
            ref = np.random.default_rng(7 + run).uniform(-2, 2, (V, F)).astype(np.float32)
            out = util.to_image(ref)
            for b in range(2):
                if b == 0:
                    ref[:, 13:F] = 0.0
                for v in range(V):
                    for k in range(K):
                        a = (C.byref(sts[v]), int(start[k, v]), int(end[k, v]), oracle.fptr(ref[v]), oracle.fptr(t0), oracle.fptr(t1))
                        if name == "nice":
                            L.zo_nice_paint(*a, int(nic[k, v]), float(sr), float(freq[k, v]), int(on[k, v]))
                        else:
                            L.zo_pmosc_paint(*a, oracle.fptr(t2), int(nic[k, v]), float(sr), float(freq[k, v]), int(on[k, v]))
                m.paint_spans(zang.Span(13, F), [out], None, float(sr), table, zero_first=b == 0)
                ctx.sync()
                assert ctx.last_form() == ["k_%s_spans%s" % (name, "_wave" if V <= 64 else "")], ctx.last_form()
                d = hc.first_difference(util.from_image(out), ref)
                if d is not None:
                    (v, f), g, w, nbad = d
                    raise AssertionError(f"{name} spans, {V} voices, sample rate {sr!r}, run {run} buffer {b}: {nbad} samples differ, first at voice {v} "
                                         f"(hostile: {where.get(v)}; sub-spans {[(int(start[k, v]), int(end[k, v])) for k in range(K)]}) frame {f}: "
                                         f"device {g!r}, oracle {w!r}")
                gs = m.state()
                words = np.zeros((V, hc.NST), np.uint32); want = np.zeros((V, hc.NST), np.uint32)
                for j, full in enumerate(desc.state):
                    a = gs
                    for part in full.replace("u:", "").split("."):
                        a = a[part]
                    words[:, j] = np.asarray(a).astype(np.uint32) if full.startswith("u:") else np.ascontiguousarray(np.asarray(a).astype(np.float32)).view(np.uint32)
                for v in range(V):
                    s = sts[v]
                    e = [s.env.state, s.env.painter.t, s.env.painter.last_value, s.env.painter.start]
                    want[v] = hc.st_bits(desc, ([s.osc.cnt, s.flt.l, s.flt.b] if name == "nice" else [s.carrier.t, s.modulator.t]) + e)
                for v in range(V):
                    assert hc.same_state(desc, words[v], want[v]), (name, V, sr, run, b, v, where.get(v), [hex(x) for x in words[v]], [hex(x) for x in want[v]])
            hs = sorted(where) if hc.bits(sr) == hc.bits(hc.SR) else list(range(V))
            compared += len(hs); nans += int(np.isnan(ref[hs]).sum()); samples += ref[hs].size
            m.close()
    assert nans <= samples // 2, (name, V, nans, samples)            # the comparison is not hollow: at most half NaN
    _report(f"{name}, span table, {V} voices", V * len(rates) * ((len(items) + per_run - 1) // per_run), compared, nans, samples)
