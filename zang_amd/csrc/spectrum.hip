// spectrum.hip -- the visualiser's FFT (examples/common/fft.zig:3-60) and the two widgets that read it (examples/visual.zig:
// DrawSpectrum.plot :257-280, DrawSpectrumFull.plot :411-452) for every voice of a [frame][voice] image, as ONE kernel:
//   k_spectrum<T, S, EPI>   a workgroup of 1,024 threads owns T consecutive voices and all n frames as complex pairs in LDS,
//                           [index][T] with the voice fastest (T = 16 at n = 1,024: 128 KiB of dynamic LDS, one workgroup per CU;
//                           T = 8: 64 KiB, two).  Row frame_start + r of the tile's voices is loaded once and stored at the
//                           bit-reversed index of r -- fftBitReverse on a power of two is that permutation -- then log2(n) stages of
//                           butterflies run on the tile, lane = (voice tid % T, butterfly slot tid / T), the twiddle pairs read from
//                           the context's table (lanes of one slot read the same pair).  S = 2: two stages per pass with a lane's
//                           four points in registers (five passes and barriers at n = 1,024; half the LDS traffic), S = 1: one.
//                           Both choices are dispatch rows; the defaults (16, 2) are the fastest pair at 4,096 and 131,072 voices.
//                           EPI: SP_FFT stores both images back in place, SP_PLOT rows 0..511 of sqrt(|re| / 1024), SP_COLUMN
//                           `height` pixels per voice from the tile's real half.
// The bits depend on each butterfly's own statements (fft_lane.hip.h zf_butterfly) and on every butterfly of a stage finishing
// before the next stage reads it; the schedule is free otherwise.  The table is the reference's f32 recurrence (zf_twiddles), built on
// the host and uploaded once per context, on first use.  Dispatch rows: spectrum_tile, spectrum_stages.  Not built: a window, n >
// 1,024, a tolerant or vendor-FFT form.
#include "common.hip.h"
#include "zmath.hip.h"
#include "fft_lane.hip.h"
#include <mutex>

enum { SP_FFT, SP_PLOT, SP_COLUMN };
// threads per workgroup.  The kernel waits on LDS latency, not on LDS bandwidth, so waves per CU decide: 1,024 threads on the 16-voice
// tile take 740 us at 131,072 voices where 256 take 1,614 and 512 take 992 (profiles/r25/NOTES.md; -DZH_SPECTRUM_BLOCK= builds the others)
#ifndef ZH_SPECTRUM_BLOCK
#define ZH_SPECTRUM_BLOCK 1024
#endif
constexpr int kSpectrumBlock = ZH_SPECTRUM_BLOCK;

struct SpectrumArgs {
    const float2 *tw;            // the n - 1 pairs (u_1, u_2), stage after stage
    uint32_t V, n, log2n;
    Img re, im;                  // row 0 = frame_start.  SP_FFT: both read and written; otherwise `re` is the samples, read only
    Img out;                     // SP_PLOT
    uint32_t *pixels;            // SP_COLUMN
    size_t row_stride;
    uint32_t height, logarithmic;
};

// A 32-lane half of a wave reads 256 bytes = one bank row with ds_read_b64: 32 / T tile rows, and which part of the bank row a tile
// row takes is its index mod 32 / T.  Neighbouring slots read rows that differ in the low bits in every pass but the first, where they
// are four rows apart: the rows' low bits are XORed with bits 2.. so that those land on different parts too.
template <int T> __device__ __forceinline__ uint32_t sp_row(uint32_t r) { return r ^ ((r >> 2) & (32 / T - 1)); }

template <int T, int S, int EPI>
__global__ void __launch_bounds__(kSpectrumBlock) k_spectrum(const SpectrumArgs a) {
    extern __shared__ float2 sp_tile[];                               // [n][T]
    constexpr uint32_t kSlots = kSpectrumBlock / T;
    const uint32_t vl = threadIdx.x % T, slot = threadIdx.x / T;
    const uint32_t v = blockIdx.x * T + vl;
    const bool live = v < a.V;                                        // a tail tile's idle lanes read and write nothing outside LDS
    const uint32_t n = a.n;
#pragma unroll 8
    for (uint32_t r = slot; r < n; r += kSlots) {
        float2 x = make_float2(0.0f, 0.0f);
        if (live) {
            x.x = *a.re.at(r, v);
            if constexpr (EPI == SP_FFT) x.y = *a.im.at(r, v);
        }
        sp_tile[sp_row<T>(zf_bit_reverse(r, a.log2n)) * T + vl] = x;
    }
    uint32_t l1 = 1;
    for (uint32_t left = a.log2n; left > 0;) {
        __syncthreads();
        if (S == 2 && left >= 2) {                                    // stages l1 and 2 l1 on the points base + {0, 1, 2, 3} l1
            const uint32_t l2 = l1 << 1;
#pragma unroll 4
            for (uint32_t g = slot; g < (n >> 2); g += kSlots) {
                const uint32_t j = g & (l1 - 1), base = ((g - j) << 2) + j;
                float2 *p0 = sp_tile + sp_row<T>(base) * T + vl, *p1 = sp_tile + sp_row<T>(base + l1) * T + vl;
                float2 *p2 = sp_tile + sp_row<T>(base + l2) * T + vl, *p3 = sp_tile + sp_row<T>(base + l2 + l1) * T + vl;
                float2 x0 = *p0, x1 = *p1, x2 = *p2, x3 = *p3;
                const float2 wa = a.tw[zf_twiddle_index(l1, j)];
                const float2 wb = a.tw[zf_twiddle_index(l2, j)], wc = a.tw[zf_twiddle_index(l2, j + l1)];
                zf_butterfly(x0.x, x0.y, x1.x, x1.y, wa.x, wa.y);
                zf_butterfly(x2.x, x2.y, x3.x, x3.y, wa.x, wa.y);
                zf_butterfly(x0.x, x0.y, x2.x, x2.y, wb.x, wb.y);
                zf_butterfly(x1.x, x1.y, x3.x, x3.y, wc.x, wc.y);
                *p0 = x0; *p1 = x1; *p2 = x2; *p3 = x3;
            }
            l1 <<= 2;
            left -= 2;
        } else {
#pragma unroll 4
            for (uint32_t g = slot; g < (n >> 1); g += kSlots) {
                const uint32_t j = g & (l1 - 1), base = ((g - j) << 1) + j;
                float2 *p0 = sp_tile + sp_row<T>(base) * T + vl, *p1 = sp_tile + sp_row<T>(base + l1) * T + vl;
                float2 x0 = *p0, x1 = *p1;
                const float2 wa = a.tw[zf_twiddle_index(l1, j)];
                zf_butterfly(x0.x, x0.y, x1.x, x1.y, wa.x, wa.y);
                *p0 = x0; *p1 = x1;
            }
            l1 <<= 1;
            left -= 1;
        }
    }
    __syncthreads();
    if (!live) return;
    if constexpr (EPI == SP_FFT) {
        for (uint32_t r = slot; r < n; r += kSlots) {
            const float2 x = sp_tile[sp_row<T>(r) * T + vl];
            *a.re.at(r, v) = x.x;
            *a.im.at(r, v) = x.y;
        }
    } else if constexpr (EPI == SP_PLOT) {
        for (uint32_t r = slot; r < kSpectrumBins; r += kSlots) *a.out.at(r, v) = zf_plot_value(sp_tile[sp_row<T>(r) * T + vl].x);
    } else {
        for (uint32_t i = slot; i < a.height; i += kSlots) {
            float f = zf_pixel_f(i, a.height);
            if (a.logarithmic) f = zf_log_position(zpowf(10.0f, f));
            const float value = zf_fft_value(f, [&](uint32_t k) ZH_INLINE_LAMBDA { return sp_tile[sp_row<T>(k) * T + vl].x; });
            a.pixels[(size_t)(a.height - 1 - i) * a.row_stride + v] = zf_pixel(value);
        }
    }
}

template <int T, int S, int EPI> static hipError_t sp_opt_in() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_spectrum<T, S, EPI>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(kFftMaxN * T * sizeof(float2)));
}
template <int T, int S> static hipError_t sp_opt_in_epilogues() {
    hipError_t e = sp_opt_in<T, S, SP_FFT>();
    if (e == hipSuccess) e = sp_opt_in<T, S, SP_PLOT>();
    if (e == hipSuccess) e = sp_opt_in<T, S, SP_COLUMN>();
    return e;
}

// The context's table: 1,023 pairs (the table of a smaller n is its prefix).  Built and uploaded at the first call on the context,
// where the kernels are also opted in to their LDS sizes (above 64 KiB at T = 16) on its device; nullptr inside a capture that would be first.
static std::mutex g_spectrum_mu;
static const float2 *spectrum_table(zh_ctx *ctx) {
    std::lock_guard<std::mutex> lk(g_spectrum_mu);
    if (ctx->fft_twiddles) return (const float2 *)ctx->fft_twiddles;
    if (ctx->capturing) return nullptr;
    static const std::vector<float> host = [] { std::vector<float> u(2 * kFftMaxN, 0.0f); zf_twiddles(u.data(), kFftMaxN); return u; }();
    if (sp_opt_in_epilogues<16, 1>() != hipSuccess || sp_opt_in_epilogues<16, 2>() != hipSuccess || sp_opt_in_epilogues<8, 1>() != hipSuccess ||
        sp_opt_in_epilogues<8, 2>() != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    void *dev = nullptr;
    if (hipMalloc(&dev, host.size() * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemcpyAsync(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(dev); return nullptr; }
    ctx->fft_twiddles = dev;
    return (const float2 *)dev;
}

template <int T, int S, int EPI> static void sp_launch(zh_ctx *ctx, const SpectrumArgs &a) {
    ZH_LAUNCH((k_spectrum<T, S, EPI>), dim3((a.V + T - 1) / T), dim3(kSpectrumBlock), (size_t)a.n * T * sizeof(float2), ctx->stream, a);
}
template <int EPI> static int sp_run(zh_ctx *ctx, SpectrumArgs &a) {
    a.tw = spectrum_table(ctx);
    if (!a.tw) return ZH_ERR_UNSUPPORTED;
    const bool narrow = zh_form(ZF_SPECTRUM_TILE) == 8, single = zh_form(ZF_SPECTRUM_STAGES) == 1;
    if (narrow) { if (single) sp_launch<8, 1, EPI>(ctx, a); else sp_launch<8, 2, EPI>(ctx, a); }
    else { if (single) sp_launch<16, 1, EPI>(ctx, a); else sp_launch<16, 2, EPI>(ctx, a); }
    return zh_launch_status();
}

static inline bool sp_pow2(uint32_t n) { return n >= 2 && n <= kFftMaxN && (n & (n - 1)) == 0; }
// rows [frame_start, frame_start + n) of all its voices lie inside the image
static inline bool sp_rows_ok(const zh_buf &b, uint32_t frame_start, uint32_t n) {
    return (uint64_t)frame_start + n <= b.frames && buf_covers(b, b.voices, frame_start + n);
}
static inline Img sp_rows(const zh_buf &b, uint32_t frame_start) { return Img{b.ptr + (size_t)frame_start * b.stride, b.stride}; }

extern "C" {

int zh_fft_twiddles(float *u, uint32_t n) {
    if (!u || !sp_pow2(n)) return ZH_ERR_INVALID;
    zf_twiddles(u, n);
    return ZH_OK;
}

int zh_fft(zh_ctx *ctx, uint32_t n, uint32_t frame_start, zh_buf re, zh_buf im) { ZH_GUARD(ctx);
    if (!ctx || !sp_pow2(n) || re.voices != im.voices) return ZH_ERR_INVALID;
    if (re.voices == 0) return ZH_OK;
    if (!sp_rows_ok(re, frame_start, n) || !sp_rows_ok(im, frame_start, n) || bufs_alias(re, im)) return ZH_ERR_INVALID;
    SpectrumArgs a{};
    a.V = re.voices; a.n = n; a.log2n = (uint32_t)__builtin_ctz(n);
    a.re = sp_rows(re, frame_start); a.im = sp_rows(im, frame_start);
    return sp_run<SP_FFT>(ctx, a);
}

int zh_spectrum_plot(zh_ctx *ctx, uint32_t frame_start, zh_buf samples, zh_buf out) { ZH_GUARD(ctx);
    if (!ctx || samples.voices != out.voices) return ZH_ERR_INVALID;
    if (samples.voices == 0) return ZH_OK;
    if (!sp_rows_ok(samples, frame_start, kFftMaxN) || !sp_rows_ok(out, 0, kSpectrumBins) || bufs_alias(samples, out)) return ZH_ERR_INVALID;
    SpectrumArgs a{};
    a.V = samples.voices; a.n = kFftMaxN; a.log2n = 10;
    a.re = sp_rows(samples, frame_start); a.out = sp_rows(out, 0);
    return sp_run<SP_PLOT>(ctx, a);
}

int zh_spectrum_column(zh_ctx *ctx, uint32_t frame_start, zh_buf samples, uint32_t *pixels, size_t row_stride_pixels, uint32_t height,
                       int logarithmic) { ZH_GUARD(ctx);
    if (!ctx || !pixels || height < 2 || row_stride_pixels < samples.voices) return ZH_ERR_INVALID;
    if (samples.voices == 0) return ZH_OK;
    if (!sp_rows_ok(samples, frame_start, kFftMaxN)) return ZH_ERR_INVALID;
    SpectrumArgs a{};
    a.V = samples.voices; a.n = kFftMaxN; a.log2n = 10;
    a.re = sp_rows(samples, frame_start);
    a.pixels = pixels; a.row_stride = row_stride_pixels; a.height = height; a.logarithmic = logarithmic ? 1u : 0u;
    return sp_run<SP_COLUMN>(ctx, a);
}

}  // extern "C"
