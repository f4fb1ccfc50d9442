// sample_kit.hip.h -- a Sampler lane whose SAMPLE is its own (src/modules/Sampler.zig:62-67: `sample` and `channel` are
// fields of Params, so they travel with every impulse: examples/example_sampler.zig:86-91, :96-105, :123-138), and the
// layout of a sample kit (zh_sample_kit: K samples of any format, channel count and native rate in one device blob), written
// once as __host__ __device__ functions so that the same text runs in a CPU harness (tests/cpp/sample_kit_lane_host.cpp).
// The lane does what SamplerLane (voices.hip.h) does, operation for operation; what differs is where the sample comes
// from: begin() loads the descriptor of THIS lane's sample index, and the PCM format is a run-time value of the lane.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include "../../include/zang_hip.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZK_HD __host__ __device__ inline
#else
#define ZK_HD inline
#endif

// ---- the kit's layout ------------------------------------------------------------------------------------------------
// Sample i's bytes start at desc[i].offset, a multiple of 4, in the order given; stray bytes after a sample's last whole
// frame are kept (they count in data_len for the wrap of Sampler.zig:133-135 and are never decoded).  A read takes the two
// aligned 32-bit words around a sample value (zk_read), so the blob ends kZkTailPad zero bytes after the last sample,
// rounded up to a word: every read of every sample stays inside it, and the blob is never shorter than two words.
constexpr size_t kZkTailPad = 8;

struct ZkSampleDesc {              // what SampleP (voices.hip.h) holds, per sample
    uint64_t offset;               // of the PCM bytes in the blob
    uint64_t data_len;             // bytes, the stray ones included
    uint32_t num_channels, sample_rate, format;
    int32_t num_samples;           // data_len / bytes_per_sample / num_channels (Sampler.zig:42)
    double inv_num_samples;        // 1.0 / num_samples (0 when there are none): zk_mod
};

inline size_t zk_round4(size_t x) { return (x + 3) & ~(size_t)3; }

// Fills desc[n] from samples[n] and returns the blob's size in *blob_bytes; ZH_ERR_INVALID for what zh_sample_kit_create refuses.
inline int zk_describe(const zh_sample *samples, uint32_t n, ZkSampleDesc *desc, size_t *blob_bytes) {
    if (!samples || n == 0) return ZH_ERR_INVALID;
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const zh_sample &s = samples[i];
        if (s.format > ZH_SAMPLE_S32_LSB || s.num_channels == 0 || (s.data_len && !s.data)) return ZH_ERR_INVALID;
        const uint64_t count = s.data_len / (s.format + 1) / s.num_channels;
        if (count > 0x7fffffffull) return ZH_ERR_INVALID;           // the reference's @intCast(i32, ...) traps (:42)
        desc[i].offset = at;
        desc[i].data_len = s.data_len;
        desc[i].num_channels = (uint32_t)s.num_channels;
        desc[i].sample_rate = (uint32_t)s.sample_rate;
        desc[i].format = s.format;
        desc[i].num_samples = (int32_t)count;
        desc[i].inv_num_samples = count > 0 ? 1.0 / (double)count : 0.0;
        at = zk_round4(at + (size_t)s.data_len);
    }
    *blob_bytes = at + kZkTailPad;
    return ZH_OK;
}
// The blob of zk_describe's layout from the samples' HOST bytes; everything between and after the samples is zero.
inline void zk_pack(const zh_sample *samples, uint32_t n, const ZkSampleDesc *desc, uint8_t *blob, size_t blob_bytes) {
    memset(blob, 0, blob_bytes);
    for (uint32_t i = 0; i < n; i++)
        if (samples[i].data_len) memcpy(blob + desc[i].offset, samples[i].data, (size_t)samples[i].data_len);
}

// ---- the lane --------------------------------------------------------------------------------------------------------
// a uint32 parameter: one value for every voice, or a device array [n_voices] (zh_u32)
struct ZkU32P {
    uint32_t value;
    const uint32_t *pv;
    ZK_HD uint32_t get(uint32_t v) const { return pv ? pv[v] : value; }
};

// @intFromFloat with NaN / out-of-range DEFINED as v_cvt_i32_f32 behaves (zmath.hip.h zf32_to_i32)
ZK_HD int32_t zk_f32_to_i32(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
#else
    if (!(v == v)) return 0;
    if (v <= -2147483648.0f) return INT32_MIN;
    if (v >= 2147483648.0f) return INT32_MAX;
    return (int32_t)v;
#endif
}
// @mod(index, n), floored (Sampler.zig:43), as voices.hip.h sampler_mod; n == 0 (inv_n == 0) gives `index` back
ZK_HD int32_t zk_mod(int32_t index, int32_t n, double inv_n) {
    const int32_t q = (int32_t)floor((double)index * inv_n);
    int32_t r = (int32_t)((uint32_t)index - (uint32_t)q * (uint32_t)n);
    r = r < 0 ? r + n : r;
    r = r >= n ? r - n : r;
    return r;
}
// the four bytes at blob + at, little-endian, from the two aligned words around them (at + 4 <= blob size - 4: the tail pad)
ZK_HD uint32_t zk_read(const uint8_t *blob, uint64_t at) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(blob + (at & ~(uint64_t)3));
    const uint64_t both = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    return (uint32_t)(both >> (8u * (uint32_t)(at & 3)));
}

struct SamplerKitLane {
    float t;                       // state (Sampler.zig:69)
    float ratio;
    int32_t t0;                    // no resampling: the rounded start position
    uint32_t n;                    // ... and frames painted so far
    bool loop, silent, plain;
    bool dead;                     // channel >= num_channels (:87-89) or no such sample: this paint() touches nothing
    // this lane's sample
    uint64_t base;                 // offset of (frame 0, channel) in the blob
    uint32_t frame_bytes;          // num_channels * bytes per value
    uint32_t shift;                // 32 - bits per value
    int32_t num_samples;
    double inv_num_samples;
    float data_len_f, inv_max;
    bool is_u8;

    // an idle lane: paints nothing until begin()
    ZK_HD void idle() {
        ratio = 0.0f; t0 = 0; n = 0; loop = false; silent = true; plain = false; dead = true;
        base = 0; frame_bytes = 0; shift = 0; num_samples = 0; inv_num_samples = 0.0; data_len_f = 0.0f; inv_max = 0.0f; is_u8 = false;
    }
    // :87-105.  A dead lane keeps everything, `t` too: the reference returns before the note_id_changed reset.
    ZK_HD void begin(const ZkSampleDesc *desc, uint32_t count, uint32_t sample, uint32_t channel, float out_rate, bool loop_,
                     bool note_id_changed) {
        silent = true; plain = false; n = 0;
        dead = sample >= count;
        if (dead) return;
        const ZkSampleDesc d = desc[sample];
        dead = channel >= d.num_channels;                             // :87-89
        if (dead) return;
        const uint32_t bytes = d.format + 1;
        base = d.offset + (uint64_t)channel * bytes;
        frame_bytes = d.num_channels * bytes;
        shift = 32 - 8 * bytes;
        is_u8 = d.format == ZH_SAMPLE_U8;
        inv_max = d.format == ZH_SAMPLE_S16_LSB ? 1.0f / 32768.0f : (d.format == ZH_SAMPLE_S24_LSB ? 1.0f / 8388608.0f : 1.0f / 2147483648.0f);
        num_samples = d.num_samples;
        inv_num_samples = d.inv_num_samples;
        data_len_f = (float)d.data_len;
        if (note_id_changed) t = 0.0f;                                // :91-93
        loop = loop_;
        ratio = (float)d.sample_rate / out_rate;                      // :97
        silent = ratio < 0.0f && !loop;                               // :99-102: nothing more (t keeps the reset)
        plain = ratio > 0.9999f && ratio < 1.0001f;                   // :105
        t0 = zk_f32_to_i32(roundf(t));
    }
    // getSample (:35-58) and decodeSigned (:23-33): outside the sample, or in an empty one, 0 and the blob's first words are read
    ZK_HD float at(const uint8_t *blob, int32_t index1) const {
        const int32_t index = loop ? zk_mod(index1, num_samples, inv_num_samples) : index1;
        const bool in = index >= 0 && index < num_samples;
        const uint32_t u = zk_read(blob, in ? base + (uint64_t)(uint32_t)index * frame_bytes : 0);
        float val;
        if (is_u8) val = ((float)(u & 0xffu) - 127.5f) / 127.5f;      // :47: a true divide
        else val = (float)((int32_t)(u << shift) >> shift) * inv_max;  // `sval / 2^(bits-1)`: one exact scaling either way
        return in ? val : 0.0f;
    }
    // one sample of :105-114 (no resampling) or :116-130 (linear); false: nothing is painted
    ZK_HD bool frame(const uint8_t *blob, float &val) {
        if (dead || silent) return false;
        if (plain) {                                                  // :107-113
            val = at(blob, (int32_t)((uint32_t)t0 + n));
            n++;
            return true;
        }
        const int32_t i0 = zk_f32_to_i32(floorf(t));                  // :117-128
        const int32_t i1 = (int32_t)((uint32_t)i0 + 1u);
        const float tfrac = (float)i1 - t;                            // :121
        const float s0 = at(blob, i0);
        const float s1 = at(blob, i1);
        val = s0 * (1.0f - tfrac) + s1 * tfrac;
        t += ratio;                                                   // :129
        return true;
    }
    ZK_HD void end() {
        if (dead || silent) return;
        if (plain) t += (float)n;                                     // :114
        if (t >= data_len_f && loop) t -= data_len_f;                 // :133-135: data.len in BYTES (reference quirk, kept)
    }
};
