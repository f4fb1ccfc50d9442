"""The yardstick of the spectrum analyser: a numpy-f32 restatement of the reference's visualiser FFT and of the two widgets that
read it, vectorised over voices (every array is [index][voice]; a voice's column never meets another's).

  examples/common/fft.zig:3-23     fftBitReverse, literally, with its h < N - 2 loop
  examples/common/fft.zig:25-60    fft: the twiddle recurrence in f32 and the three-multiply butterfly, statement by statement
  examples/visual.zig:257-280      DrawSpectrum.plot
  examples/visual.zig:141-159      getFFTValue (pow through the oracle's zo_math_powf)
  examples/visual.zig:88-125       hueToRgb / hslToRgb
  examples/visual.zig:411-452      DrawSpectrumFull.plot and its state; :127-139 scrollBlit's order

Every f32 operation is one numpy float32 operation, so each rounds once, as the reference's statements do.  DEFINED where the
reference is not, as csrc/fft_lane.hip.h states it: a float-to-u32 cast saturates and NaN casts to 0; index0 is clamped to 511;
height < 2 and n not a power of two >= 2 are refused."""
import numpy as np

F32 = np.float32
U32 = np.uint32
FRAMES = 1024
BINS = 512


def _pow2(n):
    if n < 2 or n & (n - 1):
        raise ValueError("n must be a power of two >= 2")


def bit_reverse_literal(n, re, im):
    """fft.zig:3-23 in place on [n][...] arrays"""
    i_2 = n >> 1
    j = 0
    for h in range(n - 2):
        if h < j:
            re[[h, j]] = re[[j, h]]
            im[[h, j]] = im[[j, h]]
        k = i_2
        while k <= j:
            j -= k
            k >>= 1
        j += k


def bit_reverse_permutation(n):
    """where index r stands after the plain bit-reversal permutation of n = 2^m"""
    m = n.bit_length() - 1
    return np.array([int(format(r, "0%db" % m)[::-1], 2) if m else 0 for r in range(n)], np.int64)


def twiddles(n):
    """the n - 1 pairs (u_1, u_2) fft.zig:26-58 walks through, [n - 1][2], stage after stage"""
    _pow2(n)
    out = np.zeros((n - 1, 2), F32)
    c, s = F32(-1.0), F32(0.0)
    l1, at = 1, 0
    with np.errstate(all="ignore"):
        while l1 < n:
            u_1, u_2 = F32(1.0), F32(0.0)
            for _ in range(l1):
                out[at] = (u_1, u_2)
                at += 1
                t1 = F32(F32(u_1 * c) - F32(u_2 * s))
                u_2 = F32(F32(u_1 * s) + F32(u_2 * c))
                u_1 = t1
            s = F32(-np.sqrt(F32(F32(F32(1) - c) * F32(0.5))))
            c = F32(np.sqrt(F32(F32(F32(1) + c) * F32(0.5))))
            l1 <<= 1
    return out


def fft(n, re, im):
    """fft.zig:25-60 in place on two [n][voices] f32 arrays"""
    _pow2(n)
    assert re.dtype == F32 and im.dtype == F32 and re.shape == im.shape and re.shape[0] == n
    assert re.flags.c_contiguous and im.flags.c_contiguous          # the stages work on reshaped VIEWS
    tw = twiddles(n)
    bit_reverse_literal(n, re, im)
    V = re.shape[1:]
    with np.errstate(all="ignore"):
        l1 = 1
        while l1 < n:
            l2 = l1 << 1
            u_1 = tw[l1 - 1:l2 - 1, 0].reshape((1, l1) + (1,) * len(V))
            u_2 = tw[l1 - 1:l2 - 1, 1].reshape((1, l1) + (1,) * len(V))
            r = re.reshape((n // l2, 2, l1) + V)
            i = im.reshape((n // l2, 2, l1) + V)
            rh, ri, ih, ii = r[:, 0], r[:, 1], i[:, 0], i[:, 1]          # views: point h and point h + l1 of every butterfly
            t2 = (ri - ii) * u_2
            t1 = t2 + ri * (u_1 - u_2)
            t2 = t2 + ii * (u_1 + u_2)
            r[:, 1] = rh - t1
            i[:, 1] = ih - t2
            r[:, 0] = rh + t1
            i[:, 0] = ih + t2
            l1 = l2


def fft_real(samples):
    """fft_real of a [1024][voices] block: @memcpy, @memset(fft_imag, 0), fft (visual.zig:263-265, :423-425)"""
    re = np.array(samples, F32, copy=True)
    im = np.zeros_like(re)
    fft(re.shape[0], re, im)
    return re


def plot_value(re):
    with np.errstate(all="ignore"):
        return np.sqrt(np.abs(re) * F32(1.0 / 1024.0))


def plot(samples):
    """DrawSpectrum.plot: [1024][voices] -> fft_out [512][voices]"""
    assert samples.shape[0] == FRAMES
    return plot_value(fft_real(samples)[:BINS])


def to_u32(x):
    """@intFromFloat to u32, DEFINED: NaN and everything <= 0 give 0, everything >= 2^32 gives 0xFFFFFFFF"""
    x = np.asarray(x, F32)
    out = np.zeros(x.shape, U32)
    with np.errstate(all="ignore"):
        pos = x > 0
        big = x >= F32(4294967296.0)
        mid = pos & ~big
        out[mid] = x[mid].astype(np.uint64).astype(U32)
    out[big] = U32(0xFFFFFFFF)
    return out


def oracle_pow10(oracle):
    L = oracle.lib()
    return lambda f: F32(L.zo_math_powf(10.0, float(F32(f))))


def fft_value(f, re, logarithmic, pow10):
    """getFFTValue for one position f (an f32 scalar) on [>= 512][voices] fft_real"""
    f = F32(f)
    with np.errstate(all="ignore"):
        if logarithmic:
            f = F32(F32(pow10(f) - F32(1.0)) / F32(9.0))
        f = F32(f * F32(511.5))
        f_floor = np.floor(f)
        index0 = min(int(to_u32(f_floor)), BINS - 1)
        index1 = min(BINS - 1, index0 + 1)
        frac = F32(f - f_floor)
        return re[index0] * F32(F32(1.0) - frac) + re[index1] * frac


def hue_to_rgb(p, q, t):
    with np.errstate(all="ignore"):
        t = np.where(t < 0, t + F32(1), t)
        t = np.where(t > 1, t - F32(1), t)
        a = p + (q - p) * F32(6.0) * t
        c = p + (q - p) * (F32(2.0 / 3.0) - t) * F32(6)
        return np.where(t < F32(1.0 / 6.0), a, np.where(t < F32(0.5), q, np.where(t < F32(2.0 / 3.0), c, p))).astype(F32)


def hsl_to_rgb(h, s, l):
    h = np.asarray(h, F32)
    s, l = F32(s), F32(l)
    with np.errstate(all="ignore"):
        if s == 0:
            r = g = b = np.ones_like(h)
        else:
            q = F32(l * F32(F32(1) + s)) if l < F32(0.5) else F32(F32(l + s) - F32(l * s))
            p = F32(F32(F32(2) * l) - q)
            p, q = np.full_like(h, p), np.full_like(h, q)
            r = hue_to_rgb(p, q, h + F32(1.0 / 3.0))
            g = hue_to_rgb(p, q, h)
            b = hue_to_rgb(p, q, h - F32(1.0 / 3.0))
        sqrt_h = np.sqrt(h)
        r, g, b = r * sqrt_h, g * sqrt_h, b * sqrt_h
        return U32(0xFF000000) | (to_u32(b * F32(255)) << U32(16)) | (to_u32(g * F32(255)) << U32(8)) | to_u32(r * F32(255))


def pixel(value):
    """visual.zig:432-441 for an array of blended values"""
    value = np.asarray(value, F32)
    nan = np.isnan(value)
    return np.where(nan, U32(0xFFFF0000), hsl_to_rgb(plot_value(value), 1.0, 0.5)).astype(U32)


def column(samples, height, logarithmic, pow10):
    """the column DrawSpectrumFull.plot draws, in buffer row order: [height][voices] u32, pixel i at row height - 1 - i"""
    if height < 2:
        raise ValueError("height < 2: the reference divides by height - 1")
    re = fft_real(samples)
    out = np.zeros((height,) + re.shape[1:], U32)
    for i in range(height):
        f = F32(F32(i) / F32(height - 1))
        out[height - 1 - i] = pixel(fft_value(f, re, logarithmic, pow10))
    return out


class Spectrogram:
    """DrawSpectrumFull's state for `voices` columns: buffer [height][width][voices]"""

    def __init__(self, voices, width, height, pow10):
        self.voices, self.width, self.height, self.pow10 = voices, width, height, pow10
        self.buffer = np.zeros((height, width, voices), U32)
        self.logarithmic = False
        self.drawindex = 0

    def plot(self, samples, logarithmic):
        if self.logarithmic != logarithmic:
            self.logarithmic = logarithmic
            self.buffer[:] = 0
            self.drawindex = 0
        self.buffer[:, self.drawindex, :] = column(samples, self.height, logarithmic, self.pow10)
        self.drawindex += 1
        if self.drawindex == self.width:
            self.drawindex = 0

    def scrolled(self):
        """scrollBlit: dest[w - drawindex ..] = src[0 .. drawindex], dest[0 .. w - drawindex] = src[drawindex ..]"""
        d = self.drawindex
        return np.concatenate([self.buffer[:, d:], self.buffer[:, :d]], axis=1)
