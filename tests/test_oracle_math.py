"""CPU: the oracle's libm / PRNG restatements (oracle/zmath_ref.h) against correctly rounded
values computed in float64 / exact big-integer argument reduction.  The reference takes these
from the un-vendored Zig std library: parity unpinned, accuracy pinned here."""
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_pio2_tables  # noqa: E402


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _run(L, oracle, name, xs):
    y = np.zeros_like(xs)
    getattr(L, name)(oracle.fptr(xs), oracle.fptr(y), xs.size)
    return y


def test_sin_cos_medium_range(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-900, 900, 200000), rng.uniform(-8, 8, 100000), rng.uniform(-1e-3, 1e-3, 1000),
                         np.array([0.0, -0.0, np.pi, np.pi / 2, 3 * np.pi / 4, 7 * np.pi / 4])]).astype(np.float32)
    for name, fn in (("zo_math_sinf_n", np.sin), ("zo_math_cosf_n", np.cos)):
        y = _run(L, oracle, name, xs)
        ref = fn(xs.astype(np.float64)).astype(np.float32)
        d = _ulps(y, ref)
        assert d.max() <= 1 and (d != 0).mean() < 1e-3, (name, d.max(), (d != 0).mean())


def test_sin_cos_huge_arguments_exact_reduction(oracle):
    """|x| >= 2^28*pi/2 takes the Payne-Hanek path; reduce exactly with a 600-bit pi."""
    L = oracle.lib()
    bits = 600
    pi_int = 4 * (4 * gen_pio2_tables.arctan_inv(5, bits) - gen_pio2_tables.arctan_inv(239, bits))
    twopi = Fraction(2 * pi_int, 1 << bits)
    rng = np.random.default_rng(3)
    xs = (rng.uniform(1, 2, 1500) * 2.0 ** rng.integers(29, 127, 1500)).astype(np.float32)
    xs[::2] *= -1

    def reduce(x):
        fr = Fraction(float(x))
        return float(fr - math.floor(fr / twopi) * twopi)

    red = np.array([reduce(x) for x in xs])
    for name, fn in (("zo_math_sinf_n", np.sin), ("zo_math_cosf_n", np.cos)):
        y = _run(L, oracle, name, xs)
        assert _ulps(y, fn(red).astype(np.float32)).max() <= 1
    assert math.isnan(L.zo_math_sinf(float("inf"))) and math.isnan(L.zo_math_cosf(float("nan")))


def test_sin_reduction_rint_equals_musl_ladder():
    """csrc/zmath.hip.h replaces musl's magnitude ladder (k = how many of four thresholds |x| exceeds) by
    rint(|x| * 2/pi) in float64.  Both are non-decreasing step functions of |x|, so they agree on all of
    [0, 9pi/4] iff they agree at every step point and at the ends (tools/check_sin_reduction.py sweeps all
    1.09e9 floats); a random sample rides along."""
    T = [0x3f490fda, 0x4016cbe3, 0x407b53d1, 0x40afeddf]
    invpio2 = np.float64(6.36619772367581382433e-01)
    rng = np.random.default_rng(5)
    ix = np.concatenate([np.array([0, 1, 0x00800000, 0x40e231d5], np.uint32),
                         np.array([t + d for t in T for d in range(-3, 4)], np.uint32),
                         rng.integers(0, 0x40e231d6, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    k = np.rint(ix.view(np.float32).astype(np.float64) * invpio2).astype(np.int64)
    assert np.array_equal(k, sum((ix > t).astype(np.int64) for t in T))
    # and the 1.5*2^52 trick of the medium leaf IS rint: |x * invpio2| < 2^28 there
    v = rng.uniform(-2.0 ** 28, 2.0 ** 28, 1 << 20) * invpio2
    toint = np.float64(1.5) / np.float64(2.220446049250313e-16)
    assert np.array_equal(v + toint - toint, np.rint(v))


def test_atan_pow_exp_log(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(-30, 30, 200000), rng.uniform(-1e8, 1e8, 1000)]).astype(np.float32)
    assert _ulps(_run(L, oracle, "zo_math_atanf_n", xs), np.arctan(xs.astype(np.float64)).astype(np.float32)).max() <= 1
    ys = rng.uniform(-2.0, 6.0, 200000).astype(np.float32)          # Distortion: ingain*8-2, ingain in [0,1]
    got = _run(L, oracle, "zo_math_pow2f_n", ys)
    assert _ulps(got, np.exp2(ys.astype(np.float64)).astype(np.float32)).max() <= 1
    for y, want in ((0.0, 1.0), (1.0, 2.0), (0.5, np.float32(np.sqrt(np.float32(2)))), (3.0, 8.0), (-2.0, 0.25)):
        assert np.float32(L.zo_math_powf(2.0, y)) == np.float32(want)
    es = rng.uniform(-20, 20, 50000).astype(np.float32)
    ge = np.array([L.zo_math_expf(float(x)) for x in es[:5000]], np.float32)
    assert _ulps(ge, np.exp(es[:5000].astype(np.float64)).astype(np.float32)).max() <= 1
    ls = rng.uniform(1e-6, 1e6, 5000).astype(np.float32)
    gl = np.array([L.zo_math_logf(float(x)) for x in ls], np.float32)
    assert _ulps(gl, np.log(ls.astype(np.float64)).astype(np.float32)).max() <= 1


def test_pio2_tables_rederived():
    """The 2/pi and pi/2 chunk tables pasted into zmath_ref.h / zmath.hip.h equal a fresh derivation."""
    ipio2, pio2 = gen_pio2_tables.tables()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in ("oracle/zmath_ref.h", "zang_amd/csrc/zmath.hip.h"):
        text = open(os.path.join(root, path)).read()
        for e in ipio2:
            assert ("0x%06X" % e) in text, (path, hex(e))
        for v in pio2:
            assert float.hex(v).replace("0x1.", "0x1.")[:12] in text, (path, float.hex(v))


# ------------------------------------------------------------------ pow / exp / log: the reference side of tests/test_gpu_pow.py
def _normal(a):
    b = a.view(np.uint32) & np.uint32(0x7fffffff)
    return (b >= 0x00800000) & (b <= 0x7f7fffff)


def test_exp_log_pow2_against_float64(oracle):
    """zo_math_expf_n / logf_n / powf_n(2, .) within 1 ulp of float64 rounded to f32, where the result is a normal f32 number.
    Conditions on the reference side (the device is compared with the oracle bit for bit, tests/test_gpu_pow.py)."""
    from tests import pow_cases as pc
    L = oracle.lib()
    rng = np.random.default_rng(11)
    n = 200000
    x = rng.uniform(-104.0, 89.0, n).astype(np.float32)
    with np.errstate(all="ignore"):                                            # (past 88.7 the f32 rounding is an infinity: left out below)
        got, ref = _run(L, oracle, "zo_math_expf_n", x), np.exp(x.astype(np.float64)).astype(np.float32)
    m = _normal(ref) & _normal(got)
    assert m.sum() > n * 0.8 and _ulps(got[m], ref[m]).max() <= 1, ("exp", _ulps(got[m], ref[m]).max())
    x = pc.wide_x(rng, n)                                                      # every exponent, denormals included
    assert (x.view(np.uint32) < 0x00800000).sum() > 1000
    got, ref = _run(L, oracle, "zo_math_logf_n", x), np.log(x.astype(np.float64)).astype(np.float32)
    m = _normal(ref) & _normal(got)
    assert m.sum() > n * 0.99 and _ulps(got[m], ref[m]).max() <= 1, ("log", _ulps(got[m], ref[m]).max())
    y = rng.uniform(-126.0, 127.0, n).astype(np.float32)
    got, ref = pc.oracle_pow(oracle, np.full(n, 2.0, np.float32), y), np.exp2(y.astype(np.float64)).astype(np.float32)
    m = _normal(ref) & _normal(got)
    assert m.sum() > n * 0.99 and _ulps(got[m], ref[m]).max() <= 1, ("pow(2, y)", _ulps(got[m], ref[m]).max())


def _classes(v, lo=None, hi=None):
    """0 NaN, 1 +inf, 2 -inf, 3 +0, 4 -0, 5 finite > 0, 6 finite < 0; for float64 `v` with the f32 range's ends: |v| >= hi is an
    infinity and |v| < lo a zero"""
    a = np.abs(v)
    inf = np.isinf(v) if hi is None else a >= hi
    zero = (v == 0) if lo is None else a < lo
    neg = np.signbit(v)
    c = np.where(inf, 1, np.where(zero, 3, 5)) + neg
    return np.where(np.isnan(v), 0, c)


def test_pow_result_class_against_float64(oracle):
    """General pow has no fixed ulp bound (the square-and-multiply loop rounds at every step: 8 ulps for x in [0.01, 100], |y| <= 8;
    thousands for x next to 1 and |y| in the thousands), so what is pinned is the CLASS of the result -- NaN, +-inf, +-0 with its
    sign, finite with its sign -- against float64 pow, on up to 200,000 pairs of every recipe of tests/pow_cases.py.  Pairs whose
    float64 result lies within a factor of 2 of 2^128 or 2^-150 are left out (there the loop's error may decide the class); at
    most 5 % of a recipe may go that way.

    One documented departure: finite x < 0 with |y| >= 2^31 gives NaN (the exp(y * log(x)) leaf, log of a negative number), where
    IEEE pow and Go's math.Pow -- from which Zig's std.math.pow is ported -- return 0, 1 or inf (every such y is an even integer).
    The oracle follows what its author recalled of Zig's std.math.pow (parity unpinned, no Zig std to run); this
    test records the behaviour as it is and does not decide whether the reference shares it."""
    from tests import pow_cases as pc
    rng = np.random.default_rng(12)
    seen = 0
    for name, x, y in pc.any_groups(oracle):
        if x.size > 200000:
            idx = rng.choice(x.size, 200000, replace=False)
            x, y = x[idx], y[idx]
        got = pc.oracle_pow(oracle, x, y)
        with np.errstate(all="ignore"):
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            ref = np.power(x64, y64)
        a = np.abs(ref)
        edge = ((a >= 2.0 ** 127) & (a <= 2.0 ** 129)) | ((a >= 2.0 ** -151) & (a <= 2.0 ** -149))
        assert edge.mean() <= 0.05, (name, edge.mean())
        known = np.isfinite(x) & (x < 0) & np.isfinite(y) & (np.abs(y) >= 2147483648.0)
        assert np.isnan(got[known]).all(), name
        m = ~edge & ~known
        cg, cr = _classes(got.astype(np.float64)), _classes(ref, 2.0 ** -150, 2.0 ** 128)
        bad = np.nonzero((cg != cr) & m)[0]
        assert bad.size == 0, (name, bad.size, [(float(x[i]), float(y[i]), float(got[i]), float(ref[i])) for i in bad[:8]])
        seen += int(m.sum())
    assert seen > 3_000_000


_P0, _N0, _PINF, _NINF, _ONE = 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x3f800000
_inf, _nan, _den, _big = float("inf"), float("nan"), 1.401298464324817e-45, 3.4028234663852886e+38
POW_TABLE = [  # (x, y, expected bits, or None for NaN): the special cases in the header comment of Go's math.Pow / Zig's std.math.pow
    # pow(x, +-0) = 1 for any x
    (2.0, 0.0, _ONE), (-3.0, -0.0, _ONE), (_nan, 0.0, _ONE), (_inf, -0.0, _ONE), (0.0, 0.0, _ONE), (-0.0, -0.0, _ONE), (-_inf, 0.0, _ONE),
    # pow(1, y) = 1 for any y
    (1.0, 5.0, _ONE), (1.0, _nan, _ONE), (1.0, _inf, _ONE), (1.0, -_inf, _ONE), (1.0, -0.5, _ONE),
    # pow(x, 1) = x
    (7.5, 1.0, 0x40f00000), (-2.5, 1.0, 0xc0200000), (-0.0, 1.0, _N0), (0.0, 1.0, _P0), (-_inf, 1.0, _NINF), (_den, 1.0, 0x00000001),
    # pow(NaN, y) = NaN, pow(x, NaN) = NaN
    (_nan, 2.0, None), (_nan, -_inf, None), (_nan, 1.0, None), (2.0, _nan, None), (0.0, _nan, None), (-_inf, _nan, None),
    # pow(+-0, y) = +-inf for y an odd integer < 0
    (0.0, -1.0, _PINF), (-0.0, -1.0, _NINF), (0.0, -3.0, _PINF), (-0.0, -3.0, _NINF), (-0.0, -16777215.0, _NINF),
    # pow(+-0, -inf) = +inf, pow(+-0, +inf) = +0
    (0.0, -_inf, _PINF), (-0.0, -_inf, _PINF), (0.0, _inf, _P0), (-0.0, _inf, _P0),
    # pow(+-0, y) = +inf for finite y < 0 and not an odd integer
    (0.0, -2.0, _PINF), (-0.0, -2.0, _PINF), (-0.0, -0.5, _PINF), (0.0, -1.5, _PINF), (-0.0, -16777216.0, _PINF), (-0.0, -_big, _PINF), (-0.0, -_den, _PINF),
    # pow(+-0, y) = +-0 for y an odd integer > 0
    (0.0, 3.0, _P0), (-0.0, 3.0, _N0), (-0.0, 16777215.0, _N0), (0.0, 16777215.0, _P0),
    # pow(+-0, y) = +0 for finite y > 0 and not an odd integer
    (0.0, 2.0, _P0), (-0.0, 2.0, _P0), (-0.0, 0.5, _P0), (-0.0, 1.5, _P0), (-0.0, 16777216.0, _P0), (-0.0, 16777218.0, _P0), (-0.0, _big, _P0), (-0.0, _den, _P0),
    # pow(-1, +-inf) = 1
    (-1.0, _inf, _ONE), (-1.0, -_inf, _ONE),
    # pow(x, +inf) = +inf for |x| > 1, pow(x, -inf) = +0 for |x| > 1
    (2.0, _inf, _PINF), (-2.0, _inf, _PINF), (_inf, _inf, _PINF), (-_inf, _inf, _PINF), (2.0, -_inf, _P0), (-2.0, -_inf, _P0), (-_inf, -_inf, _P0),
    # pow(x, +inf) = +0 for |x| < 1, pow(x, -inf) = +inf for |x| < 1
    (0.5, _inf, _P0), (-0.5, _inf, _P0), (_den, _inf, _P0), (0.5, -_inf, _PINF), (-0.5, -_inf, _PINF), (-_den, -_inf, _PINF),
    # pow(+inf, y) = +inf for y > 0, +0 for y < 0
    (_inf, 2.0, _PINF), (_inf, 0.5, _PINF), (_inf, _den, _PINF), (_inf, 3.0, _PINF), (_inf, -2.0, _P0), (_inf, -0.5, _P0), (_inf, -3.0, _P0), (_inf, -_den, _P0),
    # pow(-inf, y) = pow(-0, -y)
    (-_inf, 3.0, _NINF), (-_inf, 2.0, _PINF), (-_inf, 0.5, _PINF), (-_inf, 16777215.0, _NINF), (-_inf, 16777216.0, _PINF),
    (-_inf, -3.0, _N0), (-_inf, -2.0, _P0), (-_inf, -0.5, _P0), (-_inf, -16777215.0, _N0), (-_inf, -_big, _P0),
    # pow(x, y) = NaN for finite x < 0 and finite non-integer y
    (-2.0, 0.5, None), (-2.0, -0.5, None), (-2.0, 1.5, None), (-8.0, -1.0 / 3.0, None), (-_den, 2.5, None), (-_big, _den, None),
    # and around them: the sign of a negative base follows the parity of an integer y
    (-2.0, 3.0, 0xc1000000), (-2.0, 2.0, 0x40800000), (-2.0, -3.0, 0xbe000000), (-2.0, -2.0, 0x3e800000), (-1.0, 16777215.0, 0xbf800000), (-1.0, 16777216.0, _ONE),
]


def test_pow_special_case_table(oracle):
    L = oracle.lib()
    wrong = []
    for x, y, want in POW_TABLE:
        got = np.array([L.zo_math_powf(x, y)], np.float32)
        if (want is None) != bool(np.isnan(got[0])) or (want is not None and int(got.view(np.uint32)[0]) != want):
            wrong.append((x, y, want if want is None else hex(want), hex(int(got.view(np.uint32)[0]))))
    assert not wrong, wrong
    from tests import pow_cases as pc                                          # and the batch call gives the same bits, row by row
    xs, ys = np.array([r[0] for r in POW_TABLE], np.float32), np.array([r[1] for r in POW_TABLE], np.float32)
    one = np.array([L.zo_math_powf(float(a), float(b)) for a, b in zip(xs, ys)], np.float32)
    got = pc.oracle_pow(oracle, xs, ys)
    nan = np.isnan(one)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], one.view(np.uint32)[~nan])
