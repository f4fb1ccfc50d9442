// fft_lane.hip.h -- the per-element arithmetic of the spectrum analyser (spectrum.hip), written once as __host__ __device__
// functions so that the same text runs in a CPU harness (tests/cpp/fft_lane_host.cpp).  What it restates:
//   examples/common/fft.zig:3-60      the radix-2 transform: bit-reversal, then log2(n) stages of three-multiply butterflies whose
//                                     twiddles come from an f32 recurrence (up to 3.6e-4 from exp(-2 pi i j / n): the bits are the
//                                     recurrence's, no other FFT is comparable)
//   examples/visual.zig:269-271       DrawSpectrum.plot's row value, sqrt(|re| / 1024)
//   examples/visual.zig:141-159       getFFTValue: the bin position of a pixel, linear or logarithmic, and the two-bin blend
//   examples/visual.zig:88-125        hueToRgb / hslToRgb with its sqrt(h) "kludge", and the pixel word of DrawSpectrumFull.plot :429-441
// Both widgets read fft_real ONLY (:269, :430): a sine exactly on a bin shows next to nothing there, a cosine 0.7071069.  Kept.
// Cases the reference leaves undefined, DEFINED here (tests/spectrum_reference.py states the same):
//   * a float-to-u32 cast saturates and NaN casts to 0 (zf_to_u32): the channel bytes of hslToRgb, the bin index of getFFTValue
//   * index0 is clamped to 511 like index1 (no position of a height >= 2 reaches past it)
//   * height < 2 is refused (the reference divides by height - 1); n must be a power of two >= 2 (fftBitReverse underflows at 1)
// No contraction anywhere: compiled with -ffp-contract=off, every statement rounds as the reference's does.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZF_HD __host__ __device__ inline
#else
#define ZF_HD inline
#endif

constexpr uint32_t kFftMaxN = 1024;          // the largest transform, and what both plots take
constexpr uint32_t kSpectrumBins = 512;      // rows of a plot, bins a column's pixels read

// fft.zig:45-51, one butterfly of a stage: (rh, ih) = point h, (ri, ii) = point h + l1, (u1, u2) = the stage's pair for j
ZF_HD void zf_butterfly(float &rh, float &ih, float &ri, float &ii, float u1, float u2) {
    float t2 = (ri - ii) * u2;
    const float t1 = t2 + ri * (u1 - u2);
    t2 = t2 + ii * (u1 + u2);
    ri = rh - t1;
    ii = ih - t2;
    rh = rh + t1;
    ih = ih + t2;
}

// fft.zig:3-23 on a power of two n = 1 << log2n IS the bit-reversal permutation (h < N - 2 skips only self-paired and
// already-swapped indices): where element r of the input stands after it
ZF_HD uint32_t zf_bit_reverse(uint32_t r, uint32_t log2n) {
    uint32_t x = r;
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    x = (x >> 16) | (x << 16);
    return log2n ? x >> (32 - log2n) : 0;
}

// the table zh_fft_twiddles writes: stage l1 = 1, 2, 4, ... contributes l1 pairs, so its pair j stands at (l1 - 1) + j
ZF_HD uint32_t zf_twiddle_index(uint32_t l1, uint32_t j) { return l1 - 1 + j; }

// fft.zig:26-58: the n - 1 pairs (u_1, u_2) the loops walk through, by the serial f32 recurrence.  u holds 2 * (n - 1) floats
ZF_HD void zf_twiddles(float *u, uint32_t n) {
    float c = -1.0f, s = 0.0f;
    for (uint32_t l1 = 1; l1 < n; l1 <<= 1) {
        float u1 = 1.0f, u2 = 0.0f;
        for (uint32_t j = 0; j < l1; j++) {
            u[2 * zf_twiddle_index(l1, j)] = u1;
            u[2 * zf_twiddle_index(l1, j) + 1] = u2;
            const float t1 = u1 * c - u2 * s;
            u2 = u1 * s + u2 * c;
            u1 = t1;
        }
        s = -sqrtf((1.0f - c) * 0.5f);
        c = sqrtf((1.0f + c) * 0.5f);
    }
}

// @intFromFloat to u32, DEFINED: NaN and everything <= 0 give 0, everything >= 2^32 gives 0xFFFFFFFF
ZF_HD uint32_t zf_to_u32(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}

// visual.zig:269-270 (and :439): the value a bin is shown with
ZF_HD float zf_plot_value(float re) { return sqrtf(fabsf(re) * (1.0f / 1024.0f)); }

// visual.zig:429: the position of pixel i of a column, in [0, 1]
ZF_HD float zf_pixel_f(uint32_t i, uint32_t height) { return (float)i / (float)(height - 1); }
// visual.zig:144-147: the logarithmic position from 10^f (pow10f = the library's pow(10, f), zmath.hip.h zpowf on the device)
ZF_HD float zf_log_position(float pow10f) { return (pow10f - 1.0f) / 9.0f; }

// visual.zig:149-158: the blend of the two bins around position f; re_at(k) = fft_real[k], k in [0, 512)
template <class ReAt>
ZF_HD float zf_fft_value(float f, ReAt re_at) {
    f = f * 511.5f;
    const float f_floor = floorf(f);
    uint32_t index0 = zf_to_u32(f_floor);
    if (index0 > kSpectrumBins - 1) index0 = kSpectrumBins - 1;
    const uint32_t index1 = index0 + 1 < kSpectrumBins - 1 ? index0 + 1 : kSpectrumBins - 1;
    const float frac = f - f_floor;
    const float v0 = re_at(index0), v1 = re_at(index1);
    return v0 * (1.0f - frac) + v1 * frac;
}

// visual.zig:88-96; the comptime constants rounded to f32 as the reference's coercion does
ZF_HD float zf_hue_to_rgb(float p, float q, float t) {
    if (t < 0.0f) t += 1.0f;
    if (t > 1.0f) t -= 1.0f;
    if (t < (float)(1.0 / 6.0)) return p + (q - p) * 6.0f * t;
    if (t < 0.5f) return q;
    if (t < (float)(2.0 / 3.0)) return p + (q - p) * ((float)(2.0 / 3.0) - t) * 6.0f;
    return p;
}

// visual.zig:98-125, the channels' bytes overlapping where h > 1 (b << 16 wraps in 32 bits)
ZF_HD uint32_t zf_hsl_to_rgb(float h, float s, float l) {
    float r, g, b;
    if (s == 0.0f) {
        r = g = b = 1.0f;
    } else {
        const float q = l < 0.5f ? l * (1.0f + s) : l + s - l * s;
        const float p = 2.0f * l - q;
        r = zf_hue_to_rgb(p, q, h + (float)(1.0 / 3.0));
        g = zf_hue_to_rgb(p, q, h);
        b = zf_hue_to_rgb(p, q, h - (float)(1.0 / 3.0));
    }
    const float sqrt_h = sqrtf(h);
    r *= sqrt_h;
    g *= sqrt_h;
    b *= sqrt_h;
    return 0xFF000000u | (zf_to_u32(b * 255.0f) << 16) | (zf_to_u32(g * 255.0f) << 8) | zf_to_u32(r * 255.0f);
}

// visual.zig:432-441: the pixel word of one blended value
ZF_HD uint32_t zf_pixel(float fft_value) {
    if (fft_value != fft_value) return 0xFFFF0000u;
    return zf_hsl_to_rgb(zf_plot_value(fft_value), 1.0f, 0.5f);
}
