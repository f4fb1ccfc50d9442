"""CPU: tests/mix_order_reference.py, the numpy float32 restatement of the voice mixdowns' summation order, held to what can be known
without a device -- exact integer sums, the f64 sum within sqrt(V) * eps * sum |x|, the sequential order where the two must agree
and must not, planted cancellation columns whose sums are derived by hand from the documented order (tests/mix_order_cases.py), signed
zeros, and the reason the model exists: a dropped -48 dB voice that the f64 bound of the older tests accepts."""
import numpy as np
import pytest

from tests import mix_order_cases as mc
from tests import mix_order_reference as mo

F32 = np.float32
CPU_VS = sorted(set(mc.TREE_VS) - {16385, 33793} | {0, 2, 6, 63, 64, 65, 1000, 8256, 17409})
ROW_FORMS = ["wave", "workgroup"]


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ exact where every add is exact
@pytest.mark.parametrize("zero_first", [False, True])
@pytest.mark.parametrize("V", CPU_VS)
def test_tree_is_exact_on_integers(V, zero_first):
    F = 40
    src = mc.integer_image(V, F)
    dst0 = np.random.default_rng(V).integers(-1000, 1001, F).astype(F32)
    want = src.astype(np.int64).sum(axis=0) + (0 if zero_first else dst0.astype(np.int64))
    assert np.abs(want).max() < 2 ** 24
    got = mo.tree_mix(src, dst0, zero_first)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("rows_per", ROW_FORMS)
@pytest.mark.parametrize("zero_first", [False, True])
@pytest.mark.parametrize("V", [v for v in CPU_VS if v])
def test_fused_is_exact_on_integers(V, zero_first, rows_per):
    F = 40
    pv = np.ascontiguousarray(mc.integer_image(V, F).T)
    rng = np.random.default_rng(V)
    gl = rng.integers(-2, 3, V).astype(F32); gr = rng.integers(-2, 3, V).astype(F32)      # products <= 200, sums <= 200 V < 2^24
    d = [rng.integers(-1000, 1001, F).astype(F32) for _ in range(3)]
    base = [0 if zero_first else x.astype(np.int64) for x in d]
    p64 = pv.astype(np.int64)
    mono = mo.fused_mix(pv, None, d[0], zero_first, rows_per)
    left, right = mo.fused_mix(pv, (gl, gr), (d[1], d[2]), zero_first, rows_per)
    assert np.array_equal(mono.astype(np.int64), p64.sum(axis=1) + base[0])
    assert np.array_equal(left.astype(np.int64), (p64 * gl.astype(np.int64)).sum(axis=1) + base[1])
    assert np.array_equal(right.astype(np.int64), (p64 * gr.astype(np.int64)).sum(axis=1) + base[2])


# ------------------------------------------------------------------------------------------------ within sqrt(V) eps sum |x| of f64
@pytest.mark.parametrize("V", [v for v in CPU_VS if v])
def test_models_stay_within_sqrt_v_eps_of_the_f64_sum(V):
    """No factor 4.  Every result is x_i summed through a chain of d roundings at most, so |error| <= d * eps / 2 * sum |x| up to
    second order.  Tree: d = 3 (quad) + 6 (butterfly) + 3 (waves) + per + 15 (segments), and adds of +0.0 are exact -- d / 2 is below
    sqrt(V) at every V here, so the bound holds for any input.  Fused: d = 31 + 1 + 3 + rows / 128 + 127 of which the adds of dead rows
    are exact; below 64 voices d / 2 can exceed sqrt(V) and the bound holds for these seeded inputs, not for every input."""
    F = 40
    src = mc.random_image(V, F)
    zero = np.zeros(F, F32)
    ref = src.astype(np.float64).sum(axis=0)
    bound = np.sqrt(V) * mc.EPS * np.abs(src).astype(np.float64).sum(axis=0)
    assert (np.abs(mo.tree_mix(src, zero, True) - ref) <= bound).all()
    pv = np.ascontiguousarray(src.T)
    for rows_per in ROW_FORMS:
        assert (np.abs(mo.fused_mix(pv, None, zero, True, rows_per) - ref) <= bound).all(), rows_per
    g = np.random.default_rng(V).uniform(-1, 1, V).astype(F32)
    prod = (pv * g[None, :]).astype(F32).astype(np.float64)           # the products are f32 by contract; their sum is what is bounded
    left, right = mo.fused_mix(pv, (g, 1.0), (zero, zero), True, "wave")
    assert (np.abs(left - prod.sum(axis=1)) <= np.sqrt(V) * mc.EPS * np.abs(prod).sum(axis=1)).all()
    assert _same(right, mo.fused_mix(pv, None, zero, True, "wave"))     # x * 1.0f == x


# ------------------------------------------------------------------------------------------------ the order is observable
def test_tree_equals_the_sequential_order_where_the_two_coincide():
    """With zero_first (or onto zeros) the tree IS the sequential chain up to five voices: a cut quad is 0 + x0 + x1 + x2, a whole one
    ((x0 + x1) + x2) + x3, and voice 4 is alone in lane 1, which the butterfly's last step adds to lane 0: q0 + x4.  From six voices
    lane 1 holds x4 + x5 and the chain q0 + (x4 + x5) is another one.  Onto a non-zero destination the two part at two voices: the
    sequential form starts its chain at dst, (dst + x0) + x1, the tree adds dst last, dst + (x0 + x1); one voice is dst + x0 in both."""
    F = 256
    dst0 = mc.random_row(F, 3)
    for V in (1, 2, 3, 4, 5):
        src = mc.random_image(V, F)
        assert _same(mo.tree_mix(src, dst0, True), mo.sequential_mix(src, dst0, True)), V
    src = mc.random_image(1, F)
    assert _same(mo.tree_mix(src, dst0, False), mo.sequential_mix(src, dst0, False))
    assert _same(mo.tree_mix(np.zeros((0, F), F32), dst0, False), dst0)           # no voice: dst + 0.0f


@pytest.mark.parametrize("V", [3, 4, 5, 6, 64, 255, 1000, 1025])
def test_tree_differs_from_the_sequential_order(V):
    """`+=` onto a non-zero destination, three voices and more: the orders differ (docstring above) and a test that compares bits
    sees it -- in some frames at a handful of voices (two chains of three or four adds often round alike), in most from a wave up."""
    F = 256
    src = mc.random_image(V, F)
    dst0 = mc.random_row(F, 3)
    differ = _bits(mo.tree_mix(src, dst0, False)) != _bits(mo.sequential_mix(src, dst0, False))
    assert differ.any(), V
    if V >= 64:
        assert differ.mean() > 0.5, (V, differ.mean())
    if V >= 6:
        assert (_bits(mo.tree_mix(src, dst0, True)) != _bits(mo.sequential_mix(src, dst0, True))).any(), V


@pytest.mark.parametrize("V", [64, 65, 1000])
def test_fused_orders_are_three_different_orders(V):
    """per-wave rows, per-workgroup rows (from 65 voices: two live waves) and the tree are told apart by their bits"""
    F = 256
    src = mc.random_image(V, F)
    pv = np.ascontiguousarray(src.T)
    dst0 = mc.random_row(F, 4)
    wave = mo.fused_mix(pv, None, dst0, False, "wave"); wg = mo.fused_mix(pv, None, dst0, False, "workgroup")
    tree = mo.tree_mix(src, dst0, False)
    assert (_bits(wave) != _bits(tree)).mean() > 0.5
    if V >= 1000:                                  # 16 wave rows in 16 classes, 4 workgroup rows in 4: another pairing
        assert (_bits(wave) != _bits(wg)).any()
    else:                                          # one workgroup: (w0 + w1) + 0 + 0, and the classes add the same two rows
        assert _same(wave, wg)


# ------------------------------------------------------------------------------------------------ planted columns
@pytest.mark.parametrize("V", mc.PLANTED_VS + [33793])
def test_tree_planted_cancellation_columns(V):
    """1e8, 1.0 and -1e8 in one quad, in two and three lanes of a wave, in two waves and in two tiles: 0.0 or 1.0 according to where
    the three sit -- the expected values are derived in tests/mix_order_cases.py from the stated order, not by running the model.
    (33,793 voices: 34 tiles, per = 3 -- tiles 0 and 1 are both in segment 0, whose chain 0 + t0 + t1 adds them in the same order.)"""
    img, want = mc.planted_image(V)
    got = mo.tree_mix(img, np.zeros(len(want), F32), True)
    assert _same(got, want), (got, want)
    onto = mo.tree_mix(img, np.full(len(want), 0.25, F32), False)
    assert _same(onto, want + F32(0.25))


def test_fused_planted_cancellation_columns():
    """The half row is a chain: B, 1, -B in voices 0..2 is (B + 1) + -B = 0, B, -B, 1 is 1.  Across the halves of a wave: h0 = B + 1 = B,
    h1 = -B: 0, and h0 = B + -B = 0, h1 = 1: 1.  Across waves, per-wave rows: 16 rows in classes 0 .. 15, tot = (B + 1) + -B for rows 0, 1, 2 = 0; per-workgroup rows:
    ((B + 1) + -B) + 0 = 0 inside workgroup 0 as well, and B in workgroup 0, -B in workgroup 1, 1.0 in workgroup 2: (B + -B) + 1 = 1.
    A gain of -1 on the three voices flips the three signs: the same sums."""
    V, B = 1000, F32(mc.B)
    cols = [({0: B, 1: 1.0, 2: -B}, 0.0), ({0: B, 1: -B, 2: 1.0}, 1.0), ({0: B, 1: 1.0, 32: -B}, 0.0), ({0: B, 1: -B, 32: 1.0}, 1.0),
            ({0: B, 64: 1.0, 128: -B}, 0.0), ({0: B, 64: -B, 128: 1.0}, 1.0), ({0: B, 256: -B, 512: 1.0}, 1.0), ({0: B, 256: 1.0, 512: -B}, 0.0)]
    pv = np.zeros((len(cols), V), F32)
    for f, (cells, _) in enumerate(cols):
        for v, x in cells.items():
            pv[f, v] = x
    want = np.array([w for _, w in cols], F32)
    zero = np.zeros(len(cols), F32)
    for rows_per in ROW_FORMS:
        assert _same(mo.fused_mix(pv, None, zero, True, rows_per), want), rows_per
        left, right = mo.fused_mix(pv, (-1.0, 1.0), (zero, zero), True, rows_per)
        assert _same(left, -want + F32(0.0)) and _same(right, want), rows_per


# ------------------------------------------------------------------------------------------------ signed zeros
@pytest.mark.parametrize("V", [1, 4, 5, 1024, 1025, 2049])
def test_all_negative_zero_gives_positive_zero(V):
    """Both second passes start their chains at +0.0f, so an all -0.0 image gives +0.0 -- with zero_first, and onto a -0.0
    destination too: -0.0 + +0.0 = +0.0.  The same for the fused model, and for +0.0 voices times negative gains."""
    F = 9
    neg = np.full((V, F), -0.0, F32)
    pos_bits = np.zeros(F, np.uint32)
    minus = np.full(F, -0.0, F32)
    assert np.array_equal(_bits(mo.tree_mix(neg, minus, True)), pos_bits)
    assert np.array_equal(_bits(mo.tree_mix(neg, minus, False)), pos_bits)
    pv = np.ascontiguousarray(neg.T)
    for rows_per in ROW_FORMS:
        assert np.array_equal(_bits(mo.fused_mix(pv, None, minus, True, rows_per)), pos_bits)
        assert np.array_equal(_bits(mo.fused_mix(pv, None, minus, False, rows_per)), pos_bits)
        left, right = mo.fused_mix(np.zeros((F, V), F32), (-1.0, -0.0), (minus, minus), True, rows_per)
        assert np.array_equal(_bits(left), pos_bits) and np.array_equal(_bits(right), pos_bits)


def test_empty_spans_and_no_voices_write_what_the_entry_points_write():
    dst0 = mc.random_row(12, 8)
    src = mc.random_image(7, 12)
    assert _same(mo.tree_mix_span(src, dst0, 5, 5, True), dst0)                                    # nframes == 0: no launch
    none = np.zeros((0, 12), F32)
    assert _same(mo.tree_mix_span(none, dst0, 2, 9, False), dst0)                                  # dst + 0.0f: the same bits unless dst is -0.0
    want = dst0.copy(); want[2:9] = 0.0
    assert _same(mo.tree_mix_span(none, dst0, 2, 9, True), want)
    pv = np.ascontiguousarray(src.T)
    assert _same(mo.fused_mix_span(pv, None, dst0, 5, 5, True, "wave"), dst0)
    assert _same(mo.fused_mix_span(np.zeros((12, 0), F32), None, dst0, 2, 9, True, "wave"), dst0)  # zh_nice: n == 0 returns at once
    l, r = mo.fused_mix_span(pv, (1.0, 1.0), (dst0, dst0), 2, 9, False, "workgroup")
    mono = mo.fused_mix_span(pv, None, dst0, 2, 9, False, "workgroup")
    assert _same(l, mono) and _same(r, mono) and _same(mono[:2], dst0[:2]) and _same(mono[9:], dst0[9:])


# ------------------------------------------------------------------------------------------------ why the model exists
def test_the_f64_bound_accepts_a_dropped_voice_and_the_model_rejects_it():
    """1,000 voices x 256 frames (seed 9, as test_mixdown_voices): a mixdown that silently drops one voice peaking at 0.004 (-48 dB)
    misses by up to 4.0e-3.  The bound the mixdown tests had alone, 4 * sqrt(V) * eps * max(sum |x|), is 7.9e-3 here and accepts it;
    compared with the order model bit for bit, every frame is wrong."""
    V, F, seed = 1000, 256, 9
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1.0, 1.0, (V, F)).astype(F32)
    src[417] = (0.004 * np.sin(2 * np.pi * 440.0 / 48000.0 * np.arange(F) + 1.0)).astype(F32)     # the quiet voice
    dst0 = np.full(F, 0.5, F32)
    good = mo.tree_mix(src, dst0, False)
    dropped = src.copy(); dropped[417] = 0.0
    bad = mo.tree_mix(dropped, dst0, False)
    ref = 0.5 + src.astype(np.float64).sum(axis=0)
    old_bound = 4 * np.sqrt(V) * mc.EPS * np.abs(src).astype(np.float64).sum(axis=0).max()
    assert 5e-3 < old_bound < 1e-2
    miss = np.abs(bad - ref).max()
    assert 3e-3 < miss <= old_bound                                      # the old check passes a mixdown that lost a voice
    assert np.abs(good - ref).max() <= old_bound / 100                   # ... with two orders of magnitude of slack over the real error
    assert (_bits(bad) != _bits(good)).all()                             # the model's bits reject it in 256 of 256 frames
