// mix_groups.hip -- grouped sequential voice mixdown: the image's voices are n_groups groups of P consecutive voices (a voice
// bank's instruments), and every group is added in voice order in f32 -- the bits of P successive `+=` paints onto one
// buffer (examples/example_song.zig:340-346) -- into its own row, as f32 or straight through zang.mixDown's conversion
// (src/zang/mixdown.zig:28-86) into interleaved PCM.  The per-sample arithmetic is mix_lane.hip.h.
//
// Shape: the work is a read stream (4 bytes per voice-sample) with a small write.  A workgroup owns 64 frames x G groups.
// Every row's share of the tile is loaded with coalesced loads (16 bytes per lane where the layout allows) into an LDS tile
// of 64 rows, pitch 129 dwords; after a barrier thread (frame = tid % 64, wave = tid / 64) adds its groups' voices from LDS
// in order -- the 32 lanes of a ds_read_b32 group read 32 rows, which the odd pitch spreads over 32 banks -- and the 64
// lanes of a wave write 64 consecutive frames of one group.  P <= 32: G = the multiple of 4 with G * P <= 128, the tile is
// one contiguous run of G * P floats per row, wave w adds groups w, w + 4, ...  P > 32: G = 4, one group per wave, the
// voices are walked in chunks of 32 with the running sums kept in registers.  Frame tiles start at multiples of 64
// frames, so a lane's parity is its frame's: mono PCM is packed across lanes into dword stores where the row allows.
#include "common.hip.h"
#include "mix_lane.hip.h"

namespace {
constexpr uint32_t kMgFrames = 64, kMgCols = 128, kMgPitch = kMgCols + 1, kMgBlock = 256, kMgWaves = kMgBlock / 64, kMgChunk = 32;

struct MgArgs {
    const float *src;
    uint32_t stride;
    uint32_t P, G, PC;              // voices per group, groups per tile, voices of a group per chunk (P when P <= 32)
    uint32_t n_groups, n_gtiles;
    uint32_t start, end, f_base;    // the span; frame of tile row 0 of the first frame tile (start rounded down to 64)
    uint32_t vec;                   // 16-byte loads: the image's rows and every segment of a tile start 16-byte aligned
};
struct MgPcm {
    uint8_t *dst; size_t dst_stride;
    const float *acc; size_t acc_stride;
    uint32_t s16, num_channels, channel_index;
    float mul;
};

template <class Init, class Emit>
__device__ __forceinline__ void mg_tile(const MgArgs &a, float *tile, Init init, Emit emit) {
    const uint32_t tid = threadIdx.x, fl = tid % kMgFrames, w = tid / kMgFrames;
    const uint32_t gt = blockIdx.x % a.n_gtiles, ft = blockIdx.x / a.n_gtiles;
    const uint32_t g0 = gt * a.G, ng = min(a.G, a.n_groups - g0);
    const uint32_t f0 = a.f_base + ft * kMgFrames;                       // < a.end: the tile exists
    const uint32_t r_lo = a.start > f0 ? a.start - f0 : 0u, r_hi = min(a.end - f0, kMgFrames);   // the tile's rows inside the span
    const bool f_ok = fl >= r_lo && fl < r_hi;
    const uint32_t f = f0 + fl;
    // loading: tile element e of a row is voice k of segment j.  One chunk (PC == P): ONE segment, the ng * P contiguous
    // floats from column g0 * P.  Chunks: segment j = PC voices of group g0 + j, from column (g0 + j) * P + k0.
    const bool one = a.PC == a.P;
    const uint32_t seg_e = one ? a.G * a.P : a.PC, n_seg = one ? 1u : ng;
    const uint32_t per_row = a.vec ? kMgCols / 4 : kMgCols, width = a.vec ? 4u : 1u;
    const uint32_t e = (tid % per_row) * width, r0 = tid / per_row, r_step = kMgBlock / per_row;
    const uint32_t j_ld = e / seg_e, k_ld = e % seg_e;
    const float *col = a.src + (size_t)(g0 + j_ld) * a.P + k_ld;         // (dereferenced only where the checks below pass)
    float s = 0.0f;
    for (uint32_t k0 = 0; k0 < a.P; k0 += a.PC) {
        const uint32_t pc = min(a.PC, a.P - k0);
        const uint32_t seg_valid = one ? ng * a.P : pc;
        const uint32_t n_ld = (j_ld < n_seg && k_ld < seg_valid) ? min(seg_valid - k_ld, width) : 0u;
        // eight rows per thread and step: every load is issued before the first LDS store waits for one.  A row outside the
        // span is read as the nearest row inside it (the loads stay unconditional) and lands in a tile row nobody adds.
        for (uint32_t rb = r0; rb < r_hi; rb += 8 * r_step) {
            if (n_ld == 0 || rb + 7 * r_step < r_lo) continue;
            const float *p[8];
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) p[i] = col + (size_t)(f0 + min(max(rb + i * r_step, r_lo), r_hi - 1)) * a.stride + k0;
            float *t = tile + rb * kMgPitch + e;
            if (n_ld == 4) {
                float4 v[8];
#pragma unroll
                for (uint32_t i = 0; i < 8; i++) v[i] = *reinterpret_cast<const float4 *>(p[i]);
#pragma unroll
                for (uint32_t i = 0; i < 8; i++) { float *q = t + i * r_step * kMgPitch; q[0] = v[i].x; q[1] = v[i].y; q[2] = v[i].z; q[3] = v[i].w; }
            } else {
                for (uint32_t c = 0; c < n_ld; c++) {
                    float v[8];
#pragma unroll
                    for (uint32_t i = 0; i < 8; i++) v[i] = p[i][c];
#pragma unroll
                    for (uint32_t i = 0; i < 8; i++) t[i * r_step * kMgPitch + c] = v[i];
                }
            }
        }
        __syncthreads();
        for (uint32_t j = w; j < ng; j += kMgWaves) {                    // (the same trips for every lane of a wave)
            const uint32_t g = g0 + j;
            if (k0 == 0) s = f_ok ? init(g, f) : 0.0f;
            if (f_ok) s = zm_add_ordered(s, tile + fl * kMgPitch + j * a.PC, pc, 1);
            if (k0 + a.PC >= a.P) emit(g, f, fl, s, f_ok);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kMgBlock) k_mix_groups(MgArgs a, float *__restrict__ dst, size_t dst_stride, int zero_first) {
    __shared__ float tile[kMgFrames * kMgPitch];
    mg_tile(a, tile,
            [&](uint32_t g, uint32_t f) { return zero_first ? 0.0f : dst[(size_t)g * dst_stride + f]; },
            [&](uint32_t g, uint32_t f, uint32_t, float s, bool ok) { if (ok) dst[(size_t)g * dst_stride + f] = s; });
}

__global__ void __launch_bounds__(kMgBlock) k_mix_groups_pcm(MgArgs a, MgPcm o) {
    __shared__ float tile[kMgFrames * kMgPitch];
    mg_tile(a, tile,
            [&](uint32_t g, uint32_t f) { return o.acc ? o.acc[(size_t)g * o.acc_stride + f] : 0.0f; },
            [&](uint32_t g, uint32_t f, uint32_t fl, float s, bool ok) {
                const int32_t c = zm_pcm(s, o.mul, o.s16 != 0);
                uint8_t *row = o.dst + (size_t)g * o.dst_stride;
                if (o.num_channels == 1) {
                    // neighbouring frames are neighbouring lanes: 2 (s16) or 4 (s8) of them make one aligned dword
                    const uint32_t per = o.s16 ? 2u : 4u, bits = o.s16 ? 16u : 8u, mask = o.s16 ? 0xffffu : 0xffu, pos = fl & (per - 1);
                    int v = ok ? (int)(((uint32_t)c & mask) << (bits * pos)) : 0, all = ok ? 1 : 0;
                    for (uint32_t d = 1; d < per; d <<= 1) { v |= __shfl_xor(v, (int)d); all &= __shfl_xor(all, (int)d); }
                    if (!ok) return;
                    uint8_t *p = row + (size_t)f * (o.s16 ? 2 : 1);
                    if (all && ((uintptr_t)row & 3u) == 0) {
                        if (pos == 0) *reinterpret_cast<uint32_t *>(p) = (uint32_t)v;
                    } else if (o.s16) {
                        p[0] = (uint8_t)(c & 0xFF); p[1] = (uint8_t)((c >> 8) & 0xFF);
                    } else {
                        p[0] = (uint8_t)(int8_t)c;
                    }
                } else if (ok) {
                    const size_t index = (size_t)f * o.num_channels + o.channel_index;
                    if (o.s16) { row[index * 2] = (uint8_t)(c & 0xFF); row[index * 2 + 1] = (uint8_t)((c >> 8) & 0xFF); }
                    else row[index] = (uint8_t)(int8_t)c;
                }
            });
}

// the checks both entry points share; *n_groups = 0: nothing to do
int mg_prepare(zh_ctx *ctx, uint32_t start, uint32_t end, const void *dst, const zh_buf &src, uint32_t P, MgArgs *a, uint64_t *blocks) {
    if (!ctx || !dst || P == 0 || !src.ptr || src.voices % P != 0 || end < start || !buf_covers(src, src.voices, end)) return ZH_ERR_INVALID;
    a->src = src.ptr; a->stride = src.stride; a->P = P;
    a->G = P <= kMgChunk ? (kMgCols / P) & ~3u : kMgWaves;
    a->PC = P <= kMgChunk ? P : kMgChunk;
    a->n_groups = src.voices / P;
    a->n_gtiles = (a->n_groups + a->G - 1) / a->G;
    a->start = start; a->end = end; a->f_base = start & ~(kMgFrames - 1);
    // one chunk: a tile's run starts at column g0 * P, a multiple of G * P, itself a multiple of 4; chunks: at (g0 + j) * P + k0
    a->vec = (src.stride % 4 == 0 && ((uintptr_t)src.ptr & 15u) == 0 && (P <= kMgChunk || P % 4 == 0)) ? 1u : 0u;
    *blocks = (uint64_t)a->n_gtiles * (((uint64_t)end - a->f_base + kMgFrames - 1) / kMgFrames);
    return *blocks > 0x7fffffffull ? ZH_ERR_INVALID : ZH_OK;
}
}  // namespace

extern "C" {

int zh_mixdown_groups(zh_ctx *ctx, uint32_t start, uint32_t end, float *dst, size_t dst_stride_floats, zh_buf src, uint32_t group_voices,
                      uint32_t flags) { ZH_GUARD(ctx);
    MgArgs a;
    uint64_t blocks;
    int rc = mg_prepare(ctx, start, end, dst, src, group_voices, &a, &blocks);
    if (rc) return rc;
    if (a.n_groups > 1 && dst_stride_floats < end) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (a.n_groups == 0 || end == start) return ZH_OK;
    ZH_LAUNCH(k_mix_groups, dim3((uint32_t)blocks), dim3(kMgBlock), 0, ctx->stream, a, dst, dst_stride_floats, (int)(flags & ZH_PAINT_ZERO_FIRST));
    return zh_launch_status();
}

int zh_mixdown_groups_pcm(zh_ctx *ctx, uint32_t start, uint32_t end, uint8_t *dst, size_t dst_stride_bytes, zh_buf src, uint32_t group_voices,
                          const float *acc, size_t acc_stride_floats, uint32_t audio_format, uint32_t num_channels, uint32_t channel_index,
                          float vol) { ZH_GUARD(ctx);
    MgArgs a;
    uint64_t blocks;
    int rc = mg_prepare(ctx, start, end, dst, src, group_voices, &a, &blocks);
    if (rc) return rc;
    if (audio_format > ZH_AUDIO_SIGNED16_LSB || num_channels == 0 || channel_index >= num_channels) return ZH_ERR_INVALID;
    const bool s16 = audio_format == ZH_AUDIO_SIGNED16_LSB;
    if (a.n_groups > 1 && (dst_stride_bytes / num_channels / (s16 ? 2 : 1) < end || (acc && acc_stride_floats < end))) return ZH_ERR_INVALID;
    if (a.n_groups == 0 || end == start) return ZH_OK;
    const MgPcm o{dst, dst_stride_bytes, acc, acc_stride_floats, s16 ? 1u : 0u, num_channels, channel_index, zm_pcm_mul(vol, s16)};
    ZH_LAUNCH(k_mix_groups_pcm, dim3((uint32_t)blocks), dim3(kMgBlock), 0, ctx->stream, a, o);
    return zh_launch_status();
}

}  // extern "C"
