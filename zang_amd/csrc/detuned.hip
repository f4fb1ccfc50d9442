// detuned.hip -- the noise-warbled voice of examples/example_detuned.zig (:31-169) as ONE fused kernel per paint:
//   k_detuned<ZF, O1>            OuterInstrument.paint for every voice, one lane per voice (:125-168 over :53-100)
//   k_detuned_spans<ZF, O1, TB>  MainModule's Trigger loop (:213-222) for every voice from a span table, on span_walk's segments
// Lane object, frame body and the state's layout: detuned.hip.h.  O1 = outputs[1], the frequency image, is painted.  Not built: a
// few-voice form (role waves, a wave per voice, frame ranges), a tolerant form.
#include "common.hip.h"
#include "span_walk.hip.h"
#include "detuned.hip.h"
#include <vector>
#include <string.h>

struct zh_detuned {
    zh_ctx *ctx;
    uint32_t n;
    uint32_t *state;                     // [kDetunedState][n]
};

// Noise.init for voice v (Noise.zig:26-29: the (first_seed + v)-th instance); everything else starts from zero (:45-51, :117-123)
__global__ void k_detuned_seed(uint32_t *st, uint32_t n, uint64_t first_seed) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    ZXoshiro r;
    zxoshiro_seed(r, first_seed + v);
    const uint64_t s[4] = {r.s0, r.s1, r.s2, r.s3};
    for (int j = 0; j < 4; j++) { st[(size_t)(DS_RNG + 2 * j) * n + v] = (uint32_t)s[j]; st[(size_t)(DS_RNG + 2 * j + 1) * n + v] = (uint32_t)(s[j] >> 32); }
}

template <bool ZF, bool O1, class NIC>
__global__ void __launch_bounds__(kSeqBlock) k_detuned(const DetunedArgs a, const NIC nic, const Img out, const Img out1, uint32_t start, uint32_t end) {
    const uint32_t v = blockIdx.x * kSeqBlock + threadIdx.x;
    if (v >= a.V) return;
    DetunedLane n;
    n.load_state(a.state, a.V, v);
    n.begin(a, a.freq.get(v), a.note_on.get(v), a.mode.get(v), nic.get(v));
    detuned_paint_frames<ZF, O1>(n, out, out1, v, start, end, true);
    n.end();
    n.store_state(a.state, a.V, v);
}

// TB: SpanWalkP, or the table of one sub-span per voice below.  Idle lanes of the last wave shadow voice 0 read-only and store nothing.
template <bool ZF, bool O1, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_detuned_spans(const DetunedArgs a, const TB tb, const Img out, const Img out1, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    DetunedLane n;
    n.load_state(a.state, a.V, v);
    const float freq0 = a.freq.get(v);
    const uint32_t note_on0 = a.note_on.get(v) ? 1u : 0u, mode0 = a.mode.get(v);
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { n.begin(a, span_f(a.sf, kv, freq0), span_u(a.sn, kv, note_on0) != 0, span_u(a.sm, kv, mode0), nic); },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA { if (live) detuned_paint_frames<ZF, O1>(n, out, out1, v, f0, f1, active); },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}
// every voice has ONE sub-span, the span itself, with its own note_id_changed: a table that holds no arrays (zh_detuned_paint
// under the dispatch row detuned_uniform_walk)
struct DetunedOneSpanP {
    struct U32 { uint32_t x; __device__ __forceinline__ uint32_t operator[](size_t) const { return x; } };
    struct Nic { BoolP b; __device__ __forceinline__ uint8_t operator[](size_t v) const { return b.get((uint32_t)v) ? 1 : 0; } };
    uint32_t K;
    U32 count, start, end;
    Nic nic;                                                           // kv = 0 * V + v
};

// what both paints check, and the kernel's arguments
static int detuned_args(zh_detuned *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_detuned_params *p, const zh_script_span_param *sp,
                        DetunedArgs &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    if (outputs[1].ptr && !buf_covers(outputs[1], m->n, end)) return ZH_ERR_INVALID;
    a = DetunedArgs{m->n, m->state, p->sample_rate, p->patch, mk_f32(p->freq), mk_bool(p->note_on), ZkU32P{p->mode.value, p->mode.per_voice},
                    span_fa(sp, ZH_DETUNED_SPAN_FREQ), span_ua(sp, ZH_DETUNED_SPAN_NOTE_ON), span_ua(sp, ZH_DETUNED_SPAN_MODE)};
    return ZH_OK;
}

// launch NAME<zf, o1, TB> over the module's voices (TB: the table's type; k_detuned: the type of note_id_changed)
#define ZH_DETUNED_LAUNCH(NAME, ...)                                                                                      \
    do {                                                                                                                  \
        if (zf && o1) ZH_LAUNCH((NAME<true, true, __VA_ARGS__>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);        \
        else if (zf) ZH_LAUNCH((NAME<true, false, __VA_ARGS__>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);        \
        else if (o1) ZH_LAUNCH((NAME<false, true, __VA_ARGS__>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);        \
        else ZH_LAUNCH((NAME<false, false, __VA_ARGS__>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);               \
    } while (0)

extern "C" {

int zh_detuned_patch_default(zh_detuned_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_detuned_patch{4.0f, 4.0f, 0.0f, 0.75f, 0.025f, 0.1f, 1.0f, 0.5f, 880.0f, 0.8f};   // :146, :153, :71, :76, :81-84, :95, :98
    return ZH_OK;
}

int zh_detuned_create(zh_ctx *ctx, uint32_t n, uint64_t first_seed, zh_detuned **out) { ZH_GUARD(ctx);
    if (!ctx || !out) return ZH_ERR_INVALID;
    zh_detuned *m = new (std::nothrow) zh_detuned();
    if (!m) return ZH_ERR_INVALID;
    m->ctx = ctx; m->n = n; m->state = nullptr;
    int rc = dev_alloc(&m->state, (size_t)kDetunedState * n);
    if (!rc && n) { hipError_t e = hipMemsetAsync(m->state, 0, (size_t)kDetunedState * n * 4, ctx->stream); if (e != hipSuccess) rc = (int)e; }
    if (rc) { (void)hipFree(m->state); delete m; return rc; }
    if (n) ZH_LAUNCH(k_detuned_seed, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, m->state, n, first_seed);
    *out = m;
    return zh_launch_status();
}

int zh_detuned_destroy(zh_detuned *m) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->state);
    delete m;
    return ZH_OK;
}

int zh_detuned_get_state(zh_detuned *m, zh_detuned_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)kDetunedState * n);
    int rc = zh_download(m->ctx, w.data(), m->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < n; v++) ds_unpack(host[v], w.data(), n, v);
    return ZH_OK;
}

int zh_detuned_set_state(zh_detuned *m, const zh_detuned_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)kDetunedState * n);
    for (size_t v = 0; v < n; v++) ds_pack(host[v], w.data(), n, v);
    return n ? zh_upload(m->ctx, m->state, w.data(), w.size() * 4) : ZH_OK;
}

int zh_detuned_paint(zh_detuned *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                     const zh_detuned_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    DetunedArgs a;
    int rc = detuned_args(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0, o1 = outputs[1].ptr != nullptr;
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]), out1 = o1 ? mk_img(outputs[1]) : Img{nullptr, 0};
    if (zh_form(ZF_DETUNED_UNIFORM_WALK) > 0) {
        const DetunedOneSpanP tb{1, {1}, {start}, {end}, {mk_bool(note_id_changed)}};
        ZH_DETUNED_LAUNCH(k_detuned_spans, DetunedOneSpanP);
    } else {
        const BoolP tb = mk_bool(note_id_changed);
        ZH_DETUNED_LAUNCH(k_detuned, BoolP);
    }
    return zh_launch_status();
}

int zh_detuned_paint_spans(zh_detuned *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_detuned_params *p,
                           const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    static const uint8_t kinds[ZH_DETUNED_SPAN_FIELDS] = {SPAN_F, SPAN_U, SPAN_U};
    DetunedArgs a;
    int rc = detuned_args(m, start, end, outputs, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, kinds, ZH_DETUNED_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0, o1 = outputs[1].ptr != nullptr;
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]), out1 = o1 ? mk_img(outputs[1]) : Img{nullptr, 0};
    const SpanWalkP tb = mk_span_walk(table);
    ZH_DETUNED_LAUNCH(k_detuned_spans, SpanWalkP);
    return zh_launch_status();
}

}  // extern "C"
