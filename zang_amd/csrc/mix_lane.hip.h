// mix_lane.hip.h -- the per-(group, frame) arithmetic of the grouped voice mixdown (mix_groups.hip), written once as
// __host__ __device__ functions so that the same text runs in a CPU harness (tests/cpp/mix_lane_host.cpp).
// The ordered add is what P successive `+=` paints onto one buffer do (src/zang/basics.zig:31-36;
// examples/example_song.zig:340-346); the conversion is zang.mixDown's (src/zang/mixdown.zig:37-56, :66-85).
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZM_HD __host__ __device__ inline
#else
#define ZM_HD inline
#endif

// s + p[0] + p[step] + ... + p[(n - 1) * step], added in that order in f32
ZM_HD float zm_add_ordered(float s, const float *p, uint32_t n, size_t step) {
#if defined(__HIPCC__)
#pragma unroll 8
#endif
    for (uint32_t k = 0; k < n; k++) s = s + p[k * step];
    return s;
}

// mixdown.zig:37, :68 -- the factor a mixed sample is scaled by before it is clamped
ZM_HD float zm_pcm_mul(float vol, bool s16) { return vol * (s16 ? 32767.0f : 127.0f); }

// mixdown.zig:40-56 (s16) and :71-85 (s8): clamp, NaN -> 0, truncate toward zero
ZM_HD int32_t zm_pcm_s16(float value) {
    if (value <= -32767.0f) return -32767;
    if (value >= 32766.0f) return 32766;
    if (value != value) return 0;
    return (int32_t)value;
}
ZM_HD int32_t zm_pcm_s8(float value) {
    if (value <= -127.0f) return -127;
    if (value >= 126.0f) return 126;
    if (value != value) return 0;
    return (int32_t)value;
}
ZM_HD int32_t zm_pcm(float sum, float mul, bool s16) {
    const float value = sum * mul;
    return s16 ? zm_pcm_s16(value) : zm_pcm_s8(value);
}
