"""CPU: the corpus of tests/test_gpu_pow.py reaches every leaf of the device's pow / exp / log that an argument of pow can reach
(tests/pow_cases.py sorts the pairs by the inputs and the oracle's result alone), and zs_interp's pow is the oracle's batch call."""
import numpy as np
import pytest

from tests import pow_cases as pc


def test_positive_corpus_reaches_every_leaf(oracle):
    counts, pairs = pc.positive_counts(oracle)
    assert pairs >= (1 << 24) + (8 << 20)
    pc.assert_reached(counts, pc.POSITIVE_LEAVES)
    for k in set(pc.ANY_LEAVES) - set(pc.POSITIVE_LEAVES):                        # zh_pow's contract: finite x > 0
        assert counts.get(k, 0) == 0, k


def test_any_corpus_reaches_every_leaf(oracle):
    counts, pairs = pc.any_counts(oracle)
    assert pairs >= 2 * ((1 << 24) + (8 << 20)) + (2 << 20) and pairs == sum(x.size for _, x, _ in pc.any_groups(oracle))
    pc.assert_reached(counts, pc.ANY_LEAVES)


def test_a_thinned_corpus_is_noticed(oracle):
    """the conditions are not vacuous: without the integer recipe, or without the pairs aimed at zexpf's thresholds, they fail"""
    for drop in ("integer y", "zexpf leaves"):
        counts, _ = pc.corpus_counts(oracle, pc.positive_groups(oracle, sweep=False, drop=(drop,)))
        with pytest.raises(AssertionError):
            pc.assert_reached(counts, pc.POSITIVE_LEAVES)


def test_interpreter_pow_is_the_batch_call(oracle):
    """oracle/zs_interp.py computes a buffer's pow with zo_math_powf_n: the same bits as zo_math_powf pair by pair"""
    from oracle import zangscript as zs
    from oracle import zs_interp
    L = oracle.lib()
    x, y = pc.cross_product()
    s = zs.compile("P = defmodule x: waveform, y: waveform, begin out pow(x, y) end")
    out = np.full(x.size, -0.0, np.float32)                                        # -0 + r == r for every r, both zeros included
    zs_interp.make_voices(s, "P", 1, 0)[0].paint(0, x.size, out, True, [np.float32(48000), x.copy(), y.copy()])
    one = np.array([L.zo_math_powf(float(a), float(b)) for a, b in zip(x, y)], np.float32)
    nan = np.isnan(one)
    assert np.array_equal(np.isnan(out), nan) and np.array_equal(out.view(np.uint32)[~nan], one.view(np.uint32)[~nan])
    assert nan.sum() > 20 and (one.view(np.uint32) == 0x80000000).sum() >= 4      # NaN rows and negative zeros are among them
