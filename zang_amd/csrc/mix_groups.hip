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

// group tile gt, frame tile ft
template <class Init, class Emit>
__device__ __forceinline__ void mg_tile(const MgArgs &a, float *tile, uint32_t gt, uint32_t ft, Init init, Emit emit) {
    const uint32_t tid = threadIdx.x, fl = tid % kMgFrames, w = tid / kMgFrames;
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
    mg_tile(a, tile, blockIdx.x % a.n_gtiles, blockIdx.x / a.n_gtiles,
            [&](uint32_t g, uint32_t f) { return zero_first ? 0.0f : dst[(size_t)g * dst_stride + f]; },
            [&](uint32_t g, uint32_t f, uint32_t, float s, bool ok) { if (ok) dst[(size_t)g * dst_stride + f] = s; });
}

__global__ void __launch_bounds__(kMgBlock) k_mix_groups_pcm(MgArgs a, MgPcm o) {
    __shared__ float tile[kMgFrames * kMgPitch];
    mg_tile(a, tile, blockIdx.x % a.n_gtiles, blockIdx.x / a.n_gtiles,
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

// The group mix with a Decimator per group behind it (zh_decimator_paint_groups): examples/example_polyphony.zig:135-163 for every
// group -- the zeroed temps[2] the voices are added onto, then Decimator.paint (src/modules/Decimator.zig:34-56) or addInto (:162)
// onto the output.  A workgroup keeps its G groups and walks the span's frame tiles IN ORDER: what goes from frame to frame is the
// Decimator's counter alone (dcount += ratio, :46-50), which reads no sample.  Per tile thread j < G (the owner of group g0 + j's
// counter for the whole launch, in a register) runs the tile's counter steps and leaves the frames that sample as a 64-bit mask in
// LDS; the frame lanes add their group's voices as in k_mix_groups; each then takes dval from the sum of the highest sampling
// frame at or below its own (a ds_bpermute within the wave: a wave holds one group's 64 frames) or, with none, the dval carried in
// LDS, which the lane of the tile's last sampling frame then replaces.  mode: Decimator.zig:34 (0: addInto and reset), :39 (1: the
// hold), neither (2: nothing painted), and 3 = the example's bypass (:161-163: addInto, the Decimator not touched).
struct MgDec {
    float *dst; size_t dst_stride;
    const zh_group_decimation *modes;       // [n_groups]
    float *dval, *dcount;                   // [n_groups] each, updated in place: a group belongs to one workgroup
    float sample_rate;
    int zero_first;
};
__global__ void __launch_bounds__(kMgBlock) k_mix_groups_decimated(MgArgs a, MgDec d) {
    __shared__ float tile[kMgFrames * kMgPitch];
    __shared__ unsigned long long s_mask[kMgCols];
    __shared__ float s_dval[kMgCols];
    __shared__ uint32_t s_mode[kMgCols];
    const uint32_t tid = threadIdx.x, gt = blockIdx.x, g0 = gt * a.G, ng = min(a.G, a.n_groups - g0);
    uint32_t mode = 3;
    float ratio = 0.0f, dcount = 0.0f;
    if (tid < ng) {
        const zh_group_decimation md = d.modes[g0 + tid];
        mode = md.bypass ? 3u : md.fake_sample_rate >= d.sample_rate ? 0u : md.fake_sample_rate > 0.0f ? 1u : 2u;   // :34, :39
        ratio = md.fake_sample_rate / d.sample_rate;                                                                 // :40
        dcount = d.dcount[g0 + tid];
        s_dval[tid] = d.dval[g0 + tid];
        s_mode[tid] = mode;
    }
    const uint32_t n_ft = (a.end - a.f_base + kMgFrames - 1) / kMgFrames;
    for (uint32_t ft = 0; ft < n_ft; ft++) {
        if (mode == 1) {                                                 // (tid < ng) :45-50 without the sample
            const uint32_t f0 = a.f_base + ft * kMgFrames;
            const uint32_t r_lo = a.start > f0 ? a.start - f0 : 0u, r_hi = min(a.end - f0, kMgFrames);
            unsigned long long mask = 0;
            for (uint32_t r = r_lo; r < r_hi; r++) {
                const float dc = dcount + ratio;
                const bool trig = dc >= 1.0f;
                dcount = trig ? dc - 1.0f : dc;
                mask |= (unsigned long long)trig << r;
            }
            s_mask[tid] = mask;
        }
        // (mg_tile's barrier between its loads and its sums stands between the stores above and the reads below; the one after its
        // sums between those reads and the next tile's stores)
        mg_tile(a, tile, gt, ft,
                [&](uint32_t, uint32_t) { return 0.0f; },                // the zeroed temps[2], :135
                [&](uint32_t g, uint32_t f, uint32_t fl, float m, bool ok) {
                    const uint32_t j = g - g0, md = s_mode[j];           // (the same for every lane of the wave)
                    float val = m;
                    if (md == 1) {
                        const unsigned long long mask = s_mask[j], below = mask & (~0ull >> (63u - fl));
                        const float carried = s_dval[j];
                        const float held = __shfl(m, below ? 63 - __builtin_clzll(below) : (int)fl);
                        val = below ? held : carried;
                        if (mask && fl == 63u - (uint32_t)__builtin_clzll(mask)) s_dval[j] = m;   // after the wave's reads of it
                    }
                    if (!ok) return;
                    float *o = d.dst + (size_t)g * d.dst_stride + f;
                    if (md == 2) { if (d.zero_first) *o = 0.0f; }
                    else *o = (d.zero_first ? 0.0f : *o) + val;          // output[i] += ..., :51 / addInto
                });
    }
    if (tid < ng) {                                                      // (mg_tile ends on a barrier: s_dval is final)
        if (mode == 1) { d.dval[g0 + tid] = s_dval[tid]; d.dcount[g0 + tid] = dcount; }   // :54-55
        else if (mode == 0) { d.dval[g0 + tid] = 0.0f; d.dcount[g0 + tid] = 1.0f; }       // :37-38
    }
}

// the checks the entry points share; *n_groups = 0: nothing to do
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

// zh_decimator_paint_groups (modules.hip, where zh_decimator is defined) behind its NULL check
int zh_decimated_groups_launch(zh_flipper *m, uint32_t start, uint32_t end, float *dst, size_t dst_stride_floats, zh_buf src, uint32_t group_voices,
                               float sample_rate, const zh_group_decimation *modes, uint32_t flags) {
    MgArgs a;
    uint64_t blocks;
    int rc = mg_prepare(m->ctx, start, end, dst, src, group_voices, &a, &blocks);
    if (rc) return rc;
    if ((a.n_groups > 1 && dst_stride_floats < end) || m->n != a.n_groups || (a.n_groups && !modes)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (a.n_groups == 0 || end == start) return ZH_OK;
    zh_flipper_used(m);                     // a capture must know the state buffer this paint starts from (ctx.hip); in place: no flip
    float *state = reinterpret_cast<float *>(m->cnt[m->cur]);                                  // [dval n][dcount n]
    const MgDec d{dst, dst_stride_floats, modes, state, state + m->n, sample_rate, (int)(flags & ZH_PAINT_ZERO_FIRST)};
    ZH_LAUNCH(k_mix_groups_decimated, dim3(a.n_gtiles), dim3(kMgBlock), 0, m->ctx->stream, a, d);
    return zh_launch_status();
}

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
