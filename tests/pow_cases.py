"""The inputs of the pow tests (tests/test_gpu_pow.py, tests/test_pow_corpus.py, tests/test_oracle_math.py) and the proof that
they reach the code: every (x, y) pair is sorted, from the inputs and the oracle's result alone, into the leaves of zpowf_pos /
zpowf / zlogf / zexpf (csrc/zmath.hip.h, oracle/zmath_ref.h), and a count is asserted for each leaf.

No GPU here: the corpus is numpy, the only library called is the oracle (its logf places the pairs that aim at zexpf's
thresholds, and sorts pairs into zexpf's leaves)."""
import functools

import numpy as np

F32, U32 = np.float32, np.uint32
FLT_MAX, FLT_MIN, DEN_MIN, DEN_MAX, INF, NAN, ONE = 0x7f7fffff, 0x00800000, 0x00000001, 0x007fffff, 0x7f800000, 0x7fc00000, 0x3f800000
LOG_SPLIT = 0x3f3504f3                                       # zlogf: the mantissa goes to [sqrt(2)/2, sqrt(2))
EXP_THRESHOLDS = (0x39000000, 0x3eb17218, 0x3f851592)        # zexpf: 1 + x | k = 0 | k = +-1 | k from the multiply
EXP_NEAR_ULPS = 1 << 15                                      # "within 2^-8 relative" of a threshold, in ulps of the product


def fl(bits):
    return np.ascontiguousarray(np.asarray(bits, np.uint64).astype(U32)).view(F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def near(thresholds, d=4):
    """positive bit patterns t - d .. t + d of every threshold (what falls below +0 or above the last NaN is left out)"""
    out = [t + k for t in thresholds for k in range(-d, d + 1) if 0 <= t + k <= 0x7fffffff]
    return np.array(out, np.uint64)


def both_signs(pos_bits):
    return fl(np.concatenate([pos_bits, pos_bits | 0x80000000]))


def wide_x(rng, n):
    """uniform[1, 2) * 2^e, e uniform in -149..127: every exponent of f32, denormals included"""
    return (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-149, 128, n)).astype(F32)


def wide_y(rng, n):
    return (rng.uniform(-1.0, 1.0, n) * 2.0 ** rng.integers(-10, 9, n)).astype(F32)


def oracle_pow(oracle, x, y, threads=8):
    """zo_math_powf_n over the pairs (ctypes releases the GIL: the parts run side by side)"""
    import concurrent.futures as cf
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    out = np.empty_like(x)
    fn = oracle.lib().zo_math_powf_n
    n = x.size
    if threads == 1 or n < (1 << 16):
        fn(oracle.fptr(x), oracle.fptr(y), oracle.fptr(out), n)
        return out
    cuts = [n * k // threads for k in range(threads + 1)]
    with cf.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(lambda k: fn(oracle.fptr(x[cuts[k]:cuts[k + 1]]), oracle.fptr(y[cuts[k]:cuts[k + 1]]),
                                   oracle.fptr(out[cuts[k]:cuts[k + 1]]), cuts[k + 1] - cuts[k]), range(len(cuts) - 1)))
    return out


def oracle_log(oracle, x):
    x = np.ascontiguousarray(x, F32)
    out = np.empty_like(x)
    oracle.lib().zo_math_logf_n(oracle.fptr(x), oracle.fptr(out), x.size)
    return out


# ------------------------------------------------------------------ the recipes
X_SPECIAL_POS = [ONE - 1, ONE, ONE + 1, 0x40000000, 0x3f000000, FLT_MIN, DEN_MIN, DEN_MAX, FLT_MAX]
Y_THRESHOLDS = [0, 0x3f000000, ONE, 0x3fc00000, 0x40000000, 0x40200000, 0x4b000000, 0x4b800000, 0x4f000000, FLT_MAX, INF, NAN, DEN_MIN]
#               0  0.5         1    1.5         2           2.5         2^23        2^24        2^31


def pow2_sweep():
    """x = 2 against 2^24 bit patterns of y: stride 256 through all 2^32, the offset rotating from one run of 2^16 patterns to
    the next (7 is coprime to 256: all 256 residues are visited)"""
    i = np.arange(1 << 24, dtype=np.uint64)
    c = i >> 16
    y = fl(i * 256 + (c * 7 + 3) % 256)
    return np.full(y.size, 2.0, F32), y


def exp_leaf_pairs(oracle, rng, per_cell=4000):
    """pairs whose fractional path hands zexpf a product yf * log(x) within 2^-8 relative of each threshold, on both sides, both
    signs: |yf| = t / |log x| for t = T * (1 + u), |u| <= 2^-8, with |log x| >= 2.8 so that |yf| <= 0.5 even for the largest T;
    y = +-yf, and 1 - yf, 2 - yf, -(1 - yf) (yf beyond 0.5 switches to yf - 1: the product changes sign)"""
    xs, ys = [], []
    for T in EXP_THRESHOLDS:
        t = float(fl([T])[0])
        for big in (True, False):
            n = per_cell * 3
            e = rng.integers(4, 121, n) * (1 if big else -1) - (0 if big else 1)
            x = (rng.uniform(1.0, 2.0, n) * 2.0 ** e).astype(F32)
            lg = np.abs(oracle_log(oracle, x).astype(np.float64))
            yf = (t * (1.0 + rng.uniform(-1.0, 1.0, n) / 256.0) / lg).astype(F32)
            assert (yf > 0).all() and (yf < 0.5).all()
            for y in (yf, -yf, F32(1) - yf, F32(2) - yf, -(F32(1) - yf)):
                xs.append(x); ys.append(y.astype(F32))
    return np.concatenate(xs), np.concatenate(ys)


@functools.lru_cache(maxsize=None)
def _positive_groups_cached(oracle, sweep):
    rng = np.random.default_rng(20261016)
    g = []
    if sweep:
        g.append(("x = 2, stratified y",) + pow2_sweep())
    semis = np.arange(-96, 97)
    y = np.array([F32(s) / F32(12.0) for s in semis], F32)                                   # zang_amd/song.py resolve_frequencies
    g.append(("song", np.full(y.size, 2.0, F32), y))
    ingain = np.linspace(0.0, 1.0, 1 << 16).astype(F32)
    y = ingain * F32(8.0) - F32(2.0)                                                         # Distortion.zig:41
    y = np.concatenate([y, -y])
    g.append(("distortion", np.full(y.size, 2.0, F32), y))
    xr = fl(np.concatenate([rng.integers(1, FLT_MAX + 1, 300, dtype=np.uint64), np.array(X_SPECIAL_POS, np.uint64)]))
    yt = both_signs(near(Y_THRESHOLDS))
    g.append(("y thresholds", np.repeat(xr, yt.size), np.tile(yt, xr.size)))
    xt = fl(near([ONE, FLT_MIN] + [LOG_SPLIT + (e << 23) for e in (-126, -125, -100, -50, -10, -1, 0, 1, 10, 50, 100, 128)]))
    xt = xt[(bits(xt) > 0) & (bits(xt) <= FLT_MAX)]
    yr = np.concatenate([wide_y(rng, 200), rng.integers(-300, 301, 50).astype(F32), rng.uniform(-140.0, 140.0, 50).astype(F32)])
    g.append(("x thresholds", np.repeat(xt, yr.size), np.tile(yr, xt.size)))
    g.append(("zexpf leaves",) + exp_leaf_pairs(oracle, rng))
    n = 4 << 20
    g.append(("wide random", wide_x(rng, n), wide_y(rng, n)))
    n = 1 << 20
    g.append(("integer y", wide_x(rng, n), rng.integers(-300, 301, n).astype(F32)))
    g.append(("bit patterns", fl(rng.integers(1, FLT_MAX + 1, n, dtype=np.uint64)), fl(rng.integers(0, 1 << 32, n, dtype=np.uint64))))
    x, y = rng.uniform(1.5, 3.0, n).astype(F32), rng.uniform(-140.0, -80.0, n).astype(F32)
    g.append(("subnormal results", x, y))
    g.append(("subnormal results, 1 / x", (F32(1) / x).astype(F32), -y))
    for _, x, y in g:
        x.setflags(write=False); y.setflags(write=False)
        assert x.dtype == F32 and y.dtype == F32 and x.shape == y.shape and ((bits(x) >= 1) & (bits(x) <= FLT_MAX)).all()
    return tuple(g)


def positive_groups(oracle, sweep=True, drop=()):
    """[(name, x, y)]: the pairs of zh_pow's contract, finite x > 0 and any y.  `drop`: names to leave out (the thinned corpus of
    the conditions test's own test)"""
    return [t for t in _positive_groups_cached(oracle, sweep) if t[0] not in drop]


X_CROSS = [0, 0x80000000, ONE, ONE | 0x80000000, INF, INF | 0x80000000, NAN, DEN_MIN, DEN_MIN | 0x80000000, FLT_MAX, FLT_MAX | 0x80000000,
           0x40000000, 0xc0000000, 0x3f000000, 0xbf000000, 0xbf800001, 0xbf7fffff]
_Y_CROSS_POS = [0, ONE, 0x3f000000, INF, 0x40000000, 0x40400000, 0x4b7fffff, 0x4b800000, 0x4b800001, 0x4f000000, 0x3fc00000, DEN_MIN, FLT_MAX]
#               0  1    0.5         inf  2           3           2^24 - 1    2^24        2^24 + 2    2^31        1.5
Y_CROSS = _Y_CROSS_POS + [b | 0x80000000 for b in _Y_CROSS_POS] + [NAN]


def cross_product():
    x, y = fl(X_CROSS), fl(Y_CROSS)
    return np.repeat(x, y.size), np.tile(y, x.size)


@functools.lru_cache(maxsize=None)
def _extra_groups_cached():
    rng = np.random.default_rng(20261017)
    n = 1 << 20
    g = [("cross product",) + cross_product(),
         ("any bit patterns", fl(rng.integers(0, 1 << 32, n, dtype=np.uint64)), fl(rng.integers(0, 1 << 32, n, dtype=np.uint64))),
         ("negative x, integer y", -wide_x(rng, n), rng.integers(-300, 301, n).astype(F32))]
    # the rows of zpowf's tables (x == +-0, +-inf, -1, NaN) against many y: the cross product above holds each row a few times only
    xs = fl([0, 0x80000000, INF, INF | 0x80000000, ONE | 0x80000000, NAN])
    ys = np.concatenate([np.arange(-300, 301).astype(F32), wide_y(rng, 500), fl(rng.integers(0, 1 << 32, 500, dtype=np.uint64)),
                         both_signs(near([0x4b800000, 0x4f000000], d=64)), both_signs(np.array([INF], np.uint64)).repeat(50)])
    g.append(("table rows", np.repeat(xs, ys.size), np.tile(ys, xs.size)))
    for _, x, y in g:
        x.setflags(write=False); y.setflags(write=False)
    return tuple(g)


def mirrored_groups(oracle, sweep=True, drop=()):
    for name, x, y in positive_groups(oracle, sweep, drop):
        yield name + ", -x", -x, y


def extra_groups(drop=()):
    return [t for t in _extra_groups_cached() if t[0] not in drop]


def any_groups(oracle, sweep=True, drop=()):
    """the pairs of zangscript's pow(x, y), all of IEEE: every positive group with x of both signs, then the extra groups"""
    yield from positive_groups(oracle, sweep, drop)
    yield from mirrored_groups(oracle, sweep, drop)
    yield from extra_groups(drop)


# ------------------------------------------------------------------ which code a pair runs
def _odd_int(y):
    """y an odd integer below 2^24 in magnitude (the test of the x == 0 rows)"""
    ay = np.abs(y)
    small = ay < F32(16777216.0)
    yi = np.where(small, ay, 0).astype(np.int64)
    return small & (np.trunc(y) == y) & ((yi & 1) == 1)


def classify(oracle, x, y, r):
    """{leaf: pairs} for the pairs (x, y) with the oracle's result r, following zr_powf's order of tests (zmath_ref.h:370-413);
    nothing here looks at a device result"""
    c = {}
    with np.errstate(all="ignore"):
        xb, yb, rb = bits(x), bits(y), bits(r)
        xa, ra = xb & U32(0x7fffffff), rb & U32(0x7fffffff)

        def put(name, mask):
            c[name] = c.get(name, 0) + int(np.count_nonzero(mask))

        m = np.ones(x.shape, bool)

        def leave(name, mask):
            nonlocal m
            hit = m & mask
            put(name, hit)
            m = m & ~mask
            return hit

        leave("y == 0", y == 0)
        leave("x == 1", x == 1)
        put("x NaN", m & (x != x)); put("y NaN", m & (y != y))
        m = m & ~((x != x) | (y != y))
        leave("y == 1", y == 1)
        z = m & (x == 0)
        odd = _odd_int(y)
        put("x == +-0, y odd integer < 0", z & odd & (y < 0)); put("x == +-0, other y < 0", z & ~odd & (y < 0))
        put("x == +-0, y odd integer > 0", z & odd & (y > 0)); put("x == +-0, other y > 0", z & ~odd & (y > 0))
        put("x == -0", z & (xb == U32(0x80000000)))
        m = m & ~z
        yinf = m & np.isinf(y)
        put("x == -1, y == +-inf", yinf & (x == -1))
        to0 = (np.abs(x) < 1) == (y > 0)
        put("y == +-inf, result 0", yinf & (x != -1) & to0); put("y == +-inf, result inf", yinf & (x != -1) & ~to0)
        m = m & ~yinf
        xinf = m & np.isinf(x)
        put("x == +inf, y > 0", xinf & (x > 0) & (y > 0)); put("x == +inf, y < 0", xinf & (x > 0) & (y < 0))
        oddn = _odd_int(-y)
        put("x == -inf, -y odd integer < 0", xinf & (x < 0) & oddn & (y > 0)); put("x == -inf, other -y < 0", xinf & (x < 0) & ~oddn & (y > 0))
        put("x == -inf, -y odd integer > 0", xinf & (x < 0) & oddn & (y < 0)); put("x == -inf, other -y > 0", xinf & (x < 0) & ~oddn & (y < 0))
        m = m & ~xinf
        half = leave("y == 0.5", y == F32(0.5)) | leave("y == -0.5", y == F32(-0.5))
        ay = np.abs(y)
        yi = np.trunc(ay)
        yf = ay - yi
        leave("x < 0, yf != 0 (NaN)", (x < 0) & (yf != 0))
        big = leave("yi >= 2^31", yi >= F32(2147483648.0))
        put("x < 0, |y| >= 2^31 (NaN)", big & (x < 0))
        core = m
        put("yf == 0 (integer loop alone)", core & (yf == 0))
        put("0 < yf <= 0.5", core & (yf > 0) & (yf <= F32(0.5)))
        put("yf > 0.5 (yi += 1)", core & (yf > F32(0.5)))
        put("x < 0, odd integer y", core & (x < 0) & (np.mod(yi, 2) == 1)); put("x < 0, even integer y", core & (x < 0) & (np.mod(yi, 2) == 0))

        # the square-and-multiply loop: its exponent walk alone (xe doubles, less one when the squared mantissa falls below 0.5)
        sel = np.nonzero(core & (yi >= 1))[0]
        yf_s = yf[sel]
        i = (yi[sel] + (yf_s > F32(0.5))).astype(np.int64)
        x1, xe = np.frexp(x[sel])
        x1 = x1.astype(F32); xe = xe.astype(np.int64)
        broke = np.zeros(sel.size, bool)
        act = np.nonzero(i != 0)[0]
        while act.size:
            b = np.abs(xe[act]) > 512
            broke[act[b]] = True
            act = act[~b]
            sq = x1[act] * x1[act]
            e2 = xe[act] << 1
            low = sq < F32(0.5)
            x1[act] = np.where(low, sq + sq, sq); xe[act] = e2 - low
            i[act] >>= 1
            act = act[i[act] != 0]
        put("loop left by the xe break", broke)
        ys = y[sel]
        put("integer y, 3 <= |y| <= 300, loop run to its end", ~broke & (yf_s == 0) & (np.abs(ys) >= 3) & (np.abs(ys) <= 300))

        arith = half | big | core
        fin = arith & (ra < U32(INF))
        put("y < 0, finite non-zero result", fin & (y < 0) & (ra != 0))
        put("result inf by overflow", arith & (ra == U32(INF)))
        put("result 0 by underflow", arith & (ra == 0))
        put("result subnormal", arith & (ra >= 1) & (ra <= U32(DEN_MAX)))
        put("x denormal", arith & (xa >= 1) & (xa <= U32(DEN_MAX)))

        # zlogf and zexpf: called for a fractional part and for yi >= 2^31, with x > 0 (x < 0 is NaN out of zlogf's first test)
        sel = np.nonzero((big | (core & (yf != 0))) & (x > 0))[0]
        xs = x[sel]
        den = bits(xs) < U32(FLT_MIN)
        put("zlogf denormal rescale", den)
        mant = bits(np.where(den, xs * F32(33554432.0), xs).astype(F32)) & U32(0x007fffff)
        put("zlogf mantissa below the split", mant < U32(LOG_SPLIT & 0x007fffff)); put("zlogf mantissa at or above the split", mant >= U32(LOG_SPLIT & 0x007fffff))
        lg = oracle_log(oracle, xs)
        yfs = yf[sel]
        f = np.where(yfs > F32(0.5), yfs - F32(1), yfs).astype(F32)
        a = np.where(big[sel], y[sel] * lg, f * lg).astype(F32)
        ha = bits(a) & U32(0x7fffffff)
        neg = (bits(a) >> 31) == 1
        T0, T1, T2 = (U32(t) for t in EXP_THRESHOLDS)
        put("zexpf overflow", (ha >= U32(0x42b17218)) & ~neg); put("zexpf underflow", (ha >= U32(0x42cff1b5)) & neg)
        inr = ha < U32(0x42aeac50)
        put("zexpf 1 + x", ha <= T0); put("zexpf k == 0", (ha > T0) & (ha <= T1))
        put("zexpf k == +1", (ha > T1) & (ha <= T2) & ~neg); put("zexpf k == -1", (ha > T1) & (ha <= T2) & neg)
        put("zexpf |k| >= 2", (ha > T2) & inr)
        d = ha.astype(np.int64)
        for T in EXP_THRESHOLDS:
            for side, ms in (("at or below", (d <= T) & (d > T - EXP_NEAR_ULPS)), ("above", (d > T) & (d <= T + EXP_NEAR_ULPS))):
                for sg, mg in (("+", ~neg), ("-", neg)):
                    put("zexpf product within 2^-8 %s %s0x%08x" % (side, sg, T), ms & mg)
    return c


def add_counts(total, c):
    for k, v in c.items():
        total[k] = total.get(k, 0) + v
    return total


def corpus_counts(oracle, groups, threads=8, chunk=1 << 20):
    """({leaf: pairs}, pairs) over the groups.  The counts add up over pairs, so the groups are cut into chunks that are sorted side
    by side (numpy and ctypes release the GIL)"""
    import concurrent.futures as cf
    jobs = [(x[a:a + chunk], y[a:a + chunk]) for _, x, y in groups for a in range(0, x.size, chunk)]
    total = {}
    with cf.ThreadPoolExecutor(max_workers=threads) as pool:
        for c in pool.map(lambda j: classify(oracle, j[0], j[1], oracle_pow(oracle, j[0], j[1], threads=1)), jobs):
            add_counts(total, c)
    return total, sum(j[0].size for j in jobs)


@functools.lru_cache(maxsize=None)
def positive_counts(oracle):
    return corpus_counts(oracle, positive_groups(oracle))


@functools.lru_cache(maxsize=None)
def any_counts(oracle):
    """the positive groups are part of the any-corpus as they are: their counts are taken over, the rest is sorted here"""
    pos, n_pos = positive_counts(oracle)
    rest, n_rest = corpus_counts(oracle, list(mirrored_groups(oracle)) + extra_groups())
    return add_counts(dict(pos), rest), n_pos + n_rest


# ------------------------------------------------------------------ what a corpus must reach
_NEAR = {"zexpf product within 2^-8 %s %s0x%08x" % (side, sg, T): 1000 for T in EXP_THRESHOLDS for side in ("at or below", "above") for sg in "+-"}
POSITIVE_LEAVES = dict({
    "y == 0": 100, "x == 1": 100, "y NaN": 100, "y == 1": 100, "y == +-inf, result 0": 100, "y == +-inf, result inf": 100,
    "y == 0.5": 100, "y == -0.5": 100, "yi >= 2^31": 100, "yf == 0 (integer loop alone)": 100, "0 < yf <= 0.5": 100, "yf > 0.5 (yi += 1)": 100,
    "loop left by the xe break": 100, "y < 0, finite non-zero result": 100, "result inf by overflow": 100, "result 0 by underflow": 100,
    "result subnormal": 1000, "x denormal": 100, "zlogf denormal rescale": 100, "zlogf mantissa below the split": 100,
    "zlogf mantissa at or above the split": 100, "zexpf 1 + x": 100, "zexpf k == 0": 100, "zexpf k == +1": 100, "zexpf k == -1": 100,
    "zexpf |k| >= 2": 100, "zexpf overflow": 100, "zexpf underflow": 100,
    # the integer recipe alone supplies these in number (its x has every exponent, so most of its million pairs leave by the xe break;
    # about 8 % run the loop to its end): the recipe's presence is a condition of its own
    "integer y, 3 <= |y| <= 300, loop run to its end": 50000}, **_NEAR)
ANY_LEAVES = dict(POSITIVE_LEAVES, **{
    "x NaN": 100, "x == -0": 100,
    "x == +-0, y odd integer < 0": 100, "x == +-0, other y < 0": 100, "x == +-0, y odd integer > 0": 100, "x == +-0, other y > 0": 100,
    "x == -1, y == +-inf": 100,              # (only two distinct pairs exist: the table rows hold each fifty times)
    "x == +inf, y > 0": 100, "x == +inf, y < 0": 100,
    "x == -inf, -y odd integer < 0": 100, "x == -inf, other -y < 0": 100, "x == -inf, -y odd integer > 0": 100, "x == -inf, other -y > 0": 100,
    "x < 0, yf != 0 (NaN)": 100, "x < 0, |y| >= 2^31 (NaN)": 100, "x < 0, odd integer y": 100, "x < 0, even integer y": 100})
# Leaves of the device code that no argument of pow reaches (listed, not dropped silently):
#   zexpf's ldexpf(y, k) rounding into the subnormals, and its range tests between 0x42aeac50 and the overflow / underflow
#   thresholds: the fractional path calls zexpf(yf * log x) with |yf| <= 0.5 and |log x| < 104, so |product| < 52; the
#   yi >= 2^31 path calls it with |y| >= 2^31 and |log x| >= 2^-24 (x != 1), so |product| >= 128: always past the thresholds.
#   (Subnormal RESULTS of pow come from the ldexpf at the end of zpowf / zpowf_pos, which the corpus does reach.)
#   zexpf's NaN argument and zlogf's x == 0, x == inf, x == 1 returns: zpowf's tables answer those before the core.
UNREACHABLE = ("zexpf: ldexpf into the subnormals", "zexpf: 0x42aeac50 <= |x| below the overflow / underflow thresholds", "zexpf: NaN argument",
               "zlogf: x == 0, x == inf, x == 1")


def assert_reached(counts, required):
    short = {k: (counts.get(k, 0), n) for k, n in required.items() if counts.get(k, 0) < n}
    assert not short, "leaves the corpus does not reach (have, need): %r" % (short,)
