// graph_direct.hip -- what does the host-side replay of a recorded graph add to a region of a few long launches?  (round 7.)
// The kernel has the headline batch kernel's shape (k_osc_const4<.., BATCH=true>): grid (16, 64, B) x 256 threads, every lane loads
// 8 x 16 bytes of per-voice constants, computes ~100 VALU instructions per frame for 4 frames of 4 voices and stores 4 x 16 bytes
// write-through, one 16 MiB image per grid.z slice; 20 images of a 32-image (512 MiB) ring per region.  Forms:
//   graph 2x10   the two 10-buffer launches captured into a hipGraph (what a ZH_CAPTURE_COALESCE capture of 20 paints records)
//   graph 1x20   one 20-buffer launch captured into a hipGraph
//   direct 1x20  one 20-buffer launch enqueued directly (zh_graph_launch's direct replay of that capture)
//   direct 2x10  two 10-buffer launches enqueued directly
// Prints microseconds per region (median / min over the regions: wall clock from the first host call to the end of
// hipStreamSynchronize, and HIP events recorded before the first and after the last launch, as bench.py brackets its region).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

constexpr int kMaxB = 32;
struct Imgs { float *img[kMaxB]; };

__global__ void __launch_bounds__(256) k_paint_batch(const Imgs a, const uint32_t *tab, uint32_t V, uint32_t stride, uint32_t F) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t v = blockIdx.x * 256 + lane * 4;
    float *img = a.img[blockIdx.z];
    uint4 w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = *reinterpret_cast<const uint4 *>(tab + (size_t)j * V + v);
    const uint32_t chunk = blockIdx.y * 4 + wave;
    const uint32_t c0 = chunk * 4;
    const uint32_t fbase0 = blockIdx.z * F;
    uint32_t cnt[4] = {w[7].x + (fbase0 + c0) * w[0].x, w[7].y + (fbase0 + c0) * w[0].y, w[7].z + (fbase0 + c0) * w[0].z, w[7].w + (fbase0 + c0) * w[0].w};
    const uint32_t ifr[4] = {w[0].x, w[0].y, w[0].z, w[0].w};
    const float g[4] = {__uint_as_float(w[2].x), __uint_as_float(w[2].y), __uint_as_float(w[2].z), __uint_as_float(w[2].w)};
    // 4 rows of `stride` floats from row c0: c0 + 3 < F (grid.y * 16 == F), so every store stays inside the image
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(img + (size_t)c0 * stride, 0, 4u * stride * 4u, 0x00020000);
    uint32_t boff = lane * 16 + blockIdx.x * 1024;
#pragma unroll
    for (int i = 0; i < 4; i++, boff += stride * 4) {
        float val[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float p = __uint_as_float((cnt[j] >> 9) | 0x3f800000u) - 1.0f;
            float x = p;
#pragma unroll
            for (int q = 0; q < 10; q++) x = x * g[j] + (cnt[j] < ifr[j] ? p : 0.7f);      // ~25 instructions per sample
            val[j] = x;
            cnt[j] += ifr[j];
        }
        v4f acc = {val[0], val[1], val[2], val[3]};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, acc), rs, boff, 0, 16);
    }
}

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    const uint32_t V = 4096, F = 1024, K = 20, R = 32;
    const int regions = argc > 1 ? atoi(argv[1]) : 200;
    std::vector<float *> ring(R);
    for (auto &p : ring) CK(hipMalloc(&p, (size_t)V * F * 4));
    uint32_t *tab;
    CK(hipMalloc(&tab, (size_t)8 * V * 4));
    std::vector<uint32_t> h(8 * V);
    for (size_t i = 0; i < h.size(); i++) h[i] = (uint32_t)(i * 2654435761u) | 0x3f000000u;
    CK(hipMemcpy(tab, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    hipStream_t s;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

    // `n` launches of K / n buffers each, over ring images first .. first + K - 1
    auto launches = [&](uint32_t n, uint32_t first) {
        const uint32_t per = K / n;
        for (uint32_t l = 0; l < n; l++) {
            Imgs a{};
            for (uint32_t b = 0; b < per; b++) a.img[b] = ring[(first + l * per + b) % R];
            hipLaunchKernelGGL(k_paint_batch, dim3(V / 256, F / 16, per), dim3(256), 0, s, a, tab, V, V, F);
        }
    };
    auto capture = [&](uint32_t n) {
        hipGraph_t g; hipGraphExec_t ex;
        CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        launches(n, 0);
        CK(hipStreamEndCapture(s, &g));
        CK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
        return ex;
    };
    hipGraphExec_t g2 = capture(2), g1 = capture(1);

    auto measure = [&](const char *name, auto fn) {
        std::vector<double> wall, ev;
        for (int r = 0; r < regions + 20; r++) {
            CK(hipStreamSynchronize(s));
            const double t0 = now_us();
            CK(hipEventRecord(e0, s));
            fn();
            CK(hipEventRecord(e1, s));
            CK(hipStreamSynchronize(s));
            const double t1 = now_us();
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 20) { wall.push_back(t1 - t0); ev.push_back(ms * 1e3); }
        }
        std::sort(wall.begin(), wall.end()); std::sort(ev.begin(), ev.end());
        printf("%-12s wall median %7.2f min %7.2f us | events median %7.2f min %7.2f us | per buffer (events median) %.3f us = %.0f GB/s\n", name,
               wall[wall.size() / 2], wall[0], ev[ev.size() / 2], ev[0], ev[ev.size() / 2] / K, 16.777216e6 / (ev[ev.size() / 2] / K * 1e-6) / 1e9);
    };
    for (int pass = 0; pass < 2; pass++) {
        measure("graph 2x10", [&] { CK(hipGraphLaunch(g2, s)); });
        measure("graph 1x20", [&] { CK(hipGraphLaunch(g1, s)); });
        measure("direct 1x20", [&] { launches(1, 0); });
        measure("direct 2x10", [&] { launches(2, 0); });
    }
    CK(hipGetLastError());
    return 0;
}
