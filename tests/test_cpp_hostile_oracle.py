"""The hostile-parameter table (tests/hostile_cases.py) through the oracle under the sanitizers, and the conditions that keep the
device comparison of tests/test_gpu_hostile_params.py from being hollow.

tests/cpp/hostile_oracle.c and oracle/zang_oracle.c are compiled into one program of its own with
-fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all; it reads the whole table from a file and runs every
hostile record (and its ordinary counterpart) through the script.  A sanitizer report ends it with a non-zero status: the oracle
is then undefined at that record, and the record's label is in the test's message.  From its results alone, per module over the
hostile voices:
  (a) at most one half of the samples are NaN;
  (b) there are records whose paints leave the output unchanged, records with finite output that differs from the ordinary
      counterpart's, and records with NaN or an infinity in the output;
and every value of the hostile list stands in every float slot, and the ctypes oracle the device tests compare with gives the
same bits as the sanitized program."""
import os
import subprocess

import numpy as np
import pytest

from tests import hostile_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "hostile_oracle.c"), os.path.join(ROOT, "oracle", "zang_oracle.c")]
# the oracle's own flags (oracle/Makefile: no contraction, no fast math) and the sanitizers
FLAGS = ["-std=c11", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-function",
         "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]

# (module, class of (b)) the module cannot produce, with the reason
CANNOT = {
    # The echo's low-pass runs on every frame, and Filter.zig:138 subtracts its dc offset from `l` before anything is multiplied by the
    # cutoff: from a zero state the first frame's l is -2^-18 even with silence in and the filter closed (the table has both), and a
    # zeroed row (the first span) shows it.  No tuple leaves the output unchanged.
    ("FilteredEchoes", "unchanged"),
    # the same filter after the noise (which is never silent) and inside the sawtooth recipe (a voice that never plays still filters zeros)
    ("NoiseFilter", "unchanged"), ("FilteredSawtooth", "unchanged"), ("StereoEchoes", "unchanged"),
    # constant cutoff and resonance are clamped to [0, 1] (a NaN to 1) before the filter sees them, and the noise is finite
    ("NoiseFilter", "non-finite"),
    # PulseOsc paints one of two finite levels or nothing, whatever the frequency (its conversion saturates), times the Gate's 0 or 1
    ("HardSquare", "non-finite"),
    # Gate has no float: its records are the note scripts themselves, and a record differs from its counterpart in nothing
    ("Gate", "finite, differs"), ("Gate", "non-finite"),
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostile_oracle") / "hostile_oracle")
    subprocess.check_call(["gcc"] + FLAGS + SOURCES + ["-lm", "-o", exe])
    return exe


def run_harness(exe, tmp, mod, items):
    """items [(variant, rec)] -> (out [n][F], states [n][NST]); a sanitizer report fails with the records it can be among"""
    table, results = os.path.join(tmp, mod.name + ".table"), os.path.join(tmp, mod.name + ".results")
    hc.write_table(table, [(mod, va, r) for va, r in items])
    r = subprocess.run([exe, table, results], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        done = os.path.getsize(results) // (4 * hc.RESULT_WORDS) if os.path.exists(results) else 0
        at = items[min(done, len(items) - 1)]
        raise AssertionError(f"{mod.name}: the oracle harness ended with {r.returncode} near record {done} ({at[0]!r}: {at[1].label}):\n{r.stderr[-3000:]}")
    assert r.stdout.strip().endswith("PASS"), r.stdout
    return hc.read_results(results, len(items))


def unchanged_row(rec):
    """what the script leaves where no paint adds anything: the garbage with the first span zeroed"""
    row = rec.garbage.copy()
    s, e = hc.SPANS[0]
    row[s:e] = 0.0
    return row


def classify(out, rec, base_out):
    if not np.isfinite(out).all():
        return "non-finite"
    if np.array_equal(out, unchanged_row(rec)):
        return "unchanged"
    return "finite, differs" if not np.array_equal(out, base_out) else "as ordinary"


def survey(exe, tmp, mod):
    """the module's hostile records and their ordinary counterparts through the harness"""
    items = mod.all_hostile()
    both = items + [(va, r.base) for va, r in items if r.base is not None]
    out, st, ex = run_harness(exe, tmp, mod, both)
    base_out = {}
    j = len(items)
    for i, (va, r) in enumerate(items):
        if r.base is not None:
            base_out[i] = out[j]; j += 1
    return items, out[:len(items)], base_out, both, out, st, ex


@pytest.mark.parametrize("name", list(hc.MODULES))
def test_oracle_is_defined_on_the_table_and_the_table_is_worth_comparing(harness, oracle, tmp_path, name):
    mod = hc.module(name)
    items, out, base_out, both, out_all, st_all, ex_all = survey(harness, str(tmp_path), mod)
    # the ctypes oracle of the device tests computes what the sanitized program computed
    for i, (va, r) in enumerate(both):
        ref, ref_st, ref_ex = hc.reference(oracle, mod, va, r)
        assert hc.same_f32(ref, out_all[i]), (name, repr(va), r.label, hc.first_difference(ref, out_all[i]))
        assert hc.same_state(mod, ref_st, st_all[i]), (name, repr(va), r.label, ref_st, st_all[i])
        assert hc.same_f32(ref_ex, ex_all[i]), (name, repr(va), r.label, hc.first_difference(ref_ex, ex_all[i]))
    # (a)
    nan_share = float(np.isnan(out).mean())
    # (b)
    classes = {}
    for i, (va, r) in enumerate(items):
        c = classify(out[i], r, base_out.get(i))
        classes[c] = classes.get(c, 0) + 1
    print(f"{name}: {len(items)} hostile voices, NaN share {nan_share:.3f}, classes {classes}")
    assert nan_share <= 0.5, (name, nan_share)
    for c in ("unchanged", "finite, differs", "non-finite"):
        if (name, c) not in CANNOT:
            assert classes.get(c, 0) > 0, (name, c, classes)


@pytest.mark.parametrize("name", list(hc.MODULES))
def test_every_hostile_value_stands_in_every_float_slot(name):
    """every parameter slot of the module (constant and image form) and the sample rate, where the module has one"""
    mod = hc.module(name)
    want = {hc.bits(x) for x in hc.HOSTILE}
    seen = {}
    for va in mod.variants():
        if va.shared_by_paint:
            if hc.bits(va.sr) != hc.bits(hc.SR):
                seen.setdefault("sample_rate", set()).add(hc.bits(va.sr))
            continue
        for r in mod.hostile_recs(va):
            for s in mod.slots:
                x = r.p[mod.slots.index(s)]
                if hc.bits(x) != hc.bits(r.base.p[mod.slots.index(s)]):
                    seen.setdefault(s, set()).add(hc.bits(x))
            for col in ("cin", "cctl", "cc2") if " image=" in r.label else ():
                a, b = getattr(r, col).view(np.uint32), getattr(r.base, col).view(np.uint32)
                if (a != b).any():
                    seen.setdefault(f"{r.slot} image", set()).update(int(x) for x in a[a != b])
    for s in mod.slots:
        assert want <= seen.get(s, set()), (name, s)
    for s, got in seen.items():
        assert want <= got, (name, s, sorted(want - got))
    if any(hc.bits(va.sr) != hc.bits(hc.SR) for va in mod.variants()):
        assert want <= seen["sample_rate"]


def test_layout_of_a_chunk():
    """every variant but the hostile sample rates: every hostile record once alone in its group and at least once in a hostile-only
    group, and a wave that is ordinary throughout in every chunk"""
    for name in hc.MODULES:
        mod = hc.module(name)
        G = mod.group
        for va in mod.variants():
            if va.shared_by_paint:
                continue
            host = mod.hostile_recs(va)
            alone, among = [], set()
            for recs in mod.chunks(va):
                assert len(recs) == hc.V
                waves = [recs[w:w + 64] for w in range(0, hc.V, 64)]
                assert any(not any(r.hostile for r in w) for w in waves)
                for g in range(0, hc.V, G):
                    hs = [r for r in recs[g:g + G] if r.hostile]
                    if len(hs) == 1:
                        alone.append(id(hs[0]))
                    elif len(hs) == G:
                        among.update(id(r) for r in hs)
                    else:
                        assert not hs, (name, repr(va), g, len(hs))
            assert sorted(alone) == sorted(id(r) for r in host), (name, repr(va))
            assert among == {id(r) for r in host}, (name, repr(va))
