// span_walk.hip.h -- the reference's Trigger loop (src/zang/trigger.zig:80-105; examples/example_song.zig:336-347) for one
// voice: every sub-span of a per-voice table is one paint(sub_span, ..., note_id_changed, params) call.  Two walks, one contract:
// span_walk_segments (a lane per voice) under the fused instruments' span paints (composite.hip k_nice_spans / k_pmosc_spans,
// fm.hip k_fm_spans), the builtin modules' (k_<module>_spans, module_spans below) and the generated kernels' (script_rt.hip.h
// zs_span_walk); span_walk_wave (a wave per voice) under k_nice_spans_wave / k_pmosc_spans_wave.
#pragma once
#include "common.hip.h"
#include "seq.hip.h"

// The table as a walk reads it: device arrays [span][voice] (zh_script_span_table)
struct SpanWalkP {
    uint32_t K;
    const uint32_t *count, *start, *end;
    const uint8_t *nic;
};
// ... of ONE sub-span per voice, the span itself, with the voice's own note_id_changed: a table that holds no arrays (the plain
// paints that run a span kernel: zh_sampler_paint_kit, the span voices of span_voice.hip.h, zh_laser_paint)
struct OneSpanP {
    struct U32 { uint32_t x; __device__ __forceinline__ uint32_t operator[](size_t) const { return x; } };
    struct Nic { BoolP b; __device__ __forceinline__ uint8_t operator[](size_t v) const { return b.get((uint32_t)v) ? 1 : 0; } };
    uint32_t K;
    U32 count, start, end;
    Nic nic;                                                           // kv = 0 * V + v
};
// ... with the note of each sub-span (zh_span_table): the fused instruments' tables (composite.hip, fm.hip)
struct NoteSpanTableP {
    uint32_t K;
    const uint32_t *count, *start, *end;
    const float *freq;
    const uint8_t *note_on, *nic;
};

// THE CONTRACT of both walks below.  Sub-span k of voice v has its entries at kv = k * V + v; the first min(count[v], K) are read.
// A sub-span begins (prologue) at its first frame and ends (epilogue) after its last; nothing is painted between sub-spans.  A
// sub-span that starts before the previous one ends, before buf_start or after buf_end is never reached and ends the voice's
// list; one that ends before it starts, or after buf_end, runs to the buffer end without its epilogue, and nothing follows it.

// One voice per LANE.  The wave walks the buffer in segments that end at the next sub-span boundary of ANY of its lanes
// (a wave-wide minimum): inside a segment no lane starts or ends a sub-span, so the frame loop is
// the plain one of a module kernel with an `active` select -- checking every lane's boundaries on
// every frame made the first span kernel 3x slower per frame than k_nice.  Boundaries mostly coincide
// (every voice has one at each 1024-frame buffer edge), so segments are long.  `live` = the lane owns a
// voice; all 64 lanes take part in the minimum.
//   begin(kv, nic): sub-span k of voice v starts
//   segment(i, seg_end, active): frames [i, seg_end); `active` = this lane is inside a sub-span there (only a live lane is).
//   Called in EVERY lane: the callback keeps lanes that are not `live` from storing.
//   end_fn(): the sub-span ended
template <class TB, class Begin, class Segment, class End>
__device__ __forceinline__ void span_walk_segments(const TB &tb, uint32_t V, uint32_t v, bool live, uint32_t buf_start, uint32_t buf_end,
                                                   Begin &&begin, Segment &&segment, End &&end_fn) {
    const uint32_t cnt = live ? min(tb.count[v], tb.K) : 0;
    uint32_t k = 0, cur_end = 0;
    uint32_t next_start = cnt > 0 ? tb.start[v] : 0xffffffffu;
    bool active = false;
    auto advance = [&](uint32_t i) ZH_INLINE_LAMBDA {
        for (;;) {
            if (active) {
                if (i == cur_end) {
                    end_fn(); active = false; k++;
                    next_start = k < cnt ? tb.start[(size_t)k * V + v] : 0xffffffffu;
                    continue;
                }
                break;
            }
            if (i == next_start) {
                const size_t idx = (size_t)k * V + v;
                cur_end = tb.end[idx];
                begin(idx, tb.nic[idx] != 0);
                active = true;
                continue;
            }
            break;
        }
    };
    uint32_t i = buf_start;
    while (i < buf_end) {
        advance(i);                                             // sub-spans that end / begin at frame i
        uint32_t ev = active ? cur_end : next_start;            // this lane's next boundary (> i)
        ev = (ev > i && ev < buf_end) ? ev : buf_end;           // unsorted / out-of-range entries never fire
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ev = min(ev, (uint32_t)__shfl_xor((int)ev, off));
        const uint32_t seg_end = __builtin_amdgcn_readfirstlane(ev);
        segment(i, seg_end, active);
        i = seg_end;
    }
    advance(buf_end);          // a sub-span that ends with the buffer; empty sub-spans at buf_end
}

// span_walk_segments over the frame loop of a module kernel (seq.hip.h frame_loop, 8-frame chunks):
//   frame(x, val) -> painted: one frame of an active sub-span, x = the NIN input images' samples at the ABSOLUTE frame
template <bool ZF, int NIN, class TB, class Begin, class Frame, class End>
__device__ __forceinline__ void span_walk(const TB &tb, uint32_t V, uint32_t v, bool live, Img out, const float *const *in,
                                          const size_t *istr, uint32_t buf_start, uint32_t buf_end, Begin &&begin, Frame &&frame,
                                          End &&end_fn) {
    span_walk_segments(tb, V, v, live, buf_start, buf_end, begin,
                       [&](uint32_t i, uint32_t seg_end, bool active) ZH_INLINE_LAMBDA {
        if (live) {
            frame_loop<8, ZF, NIN>(out.p, v, out.stride, in, istr, i, seg_end,
                                   [&](uint32_t, const float (&x)[NIN > 0 ? NIN : 1], float &val) ZH_INLINE_LAMBDA {
                if (!active) return false;
                return (bool)frame(x, val);
            });
        }
    }, end_fn);
}

// One voice per WAVE, its lanes 64 consecutive frames (the fused instruments at a handful of voices: composite.hip
// k_nice_spans_wave / k_pmosc_spans_wave).  Frames outside the sub-spans are zeroed here (ZF); a sub-span is handed over in
// blocks of up to 64 frames.
//   begin(kv): sub-span k starts (the kernel reads the table's other arrays at kv itself)
//   block(f0, nf): frames [f0, f0 + nf), nf <= 64, lane j = frame f0 + j
//   end_fn(): the sub-span ended
template <bool ZF, class TB, class Begin, class Block, class End>
__device__ __forceinline__ void span_walk_wave(const TB &tb, uint32_t V, uint32_t v, uint32_t lane, Img out, uint32_t buf_start,
                                               uint32_t buf_end, Begin &&begin, Block &&block, End &&end_fn) {
    const uint32_t cnt = min(tb.count[v], tb.K);
    float *col = out.p + v;
    const size_t os = out.stride;
    auto zero = [&](uint32_t f0, uint32_t f1) ZH_INLINE_LAMBDA {
        if (ZF) for (uint32_t f = f0 + lane; f < f1; f += 64) col[(size_t)f * os] = 0.0f;
    };
    uint32_t i = buf_start;
    for (uint32_t k = 0; k < cnt; k++) {
        const size_t idx = (size_t)k * V + v;
        const uint32_t s0 = tb.start[idx], s1 = tb.end[idx];
        if (s0 < i || s0 > buf_end) break;                      // never reached in order: nothing further fires
        zero(i, s0);
        begin(idx);
        const bool ends = s1 >= s0 && s1 <= buf_end;            // otherwise the sub-span runs to the buffer end, unfinished
        const uint32_t seg_end = ends ? s1 : buf_end;
        for (uint32_t f0 = s0; f0 < seg_end; f0 += 64) block(f0, min(64u, seg_end - f0));
        i = seg_end;
        if (!ends) break;
        end_fn();
    }
    zero(i, buf_end);
}

#if !defined(ZH_DEVICE_ONLY)   // the rest is the library's own: the generated kernels' runtime (hiprtc) takes the walks alone
// One builtin module's span paint, one lane per voice (kSeqBlock-lane blocks over seq_grid(V)).  The adapter A wraps the
// module's lane object (voices.hip.h):
//   A::Args                          the kernel's argument block (a.V = voices); the per-sub-span arrays ride in it
//   A::NIN                           input images read at the absolute frame (Filter / Decimator / Distortion input, cob buffers)
//   load(a, v) / store(a, v)         the voice's state, and the values of the fields that have no span array
//   inputs(a, in, istr)              the NIN input images
//   begin(a, kv, nic) / frame(a, x, val) -> painted / end(a)   one paint() call's prologue, frames and epilogue
// Idle lanes of the last wave shadow voice 0 read-only and store nothing.
// TB: the table, SpanWalkP or anything that reads like it (OneSpanP: one sub-span per voice, no arrays).
template <bool ZF, class A, class TB>
__device__ __forceinline__ void module_spans(const typename A::Args &a, const TB &tb, Img out, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    constexpr int NI = A::NIN > 0 ? A::NIN : 1;
    const float *ins[NI];
    size_t istr[NI];
#pragma unroll
    for (int j = 0; j < NI; j++) { ins[j] = nullptr; istr[j] = 0; }
    A m;
    m.load(a, v);
    m.inputs(a, ins, istr);
    span_walk<ZF, A::NIN>(tb, a.V, v, live, out, ins, istr, start, end,
                          [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { m.begin(a, kv, nic); },
                          [&](const float (&x)[NI], float &val) ZH_INLINE_LAMBDA { return m.frame(a, x, val); },
                          [&]() ZH_INLINE_LAMBDA { m.end(a); });
    if (live) m.store(a, v);
}
// the stable kernel name of one module's span paint (zh_last_form, rocprofv3): NAME<ZF, Adapter>
#define ZH_MODULE_SPANS_KERNEL(NAME)                                                                                       \
    template <bool ZF, class A>                                                                                           \
    __global__ void __launch_bounds__(kSeqBlock) NAME(const typename A::Args a, const SpanWalkP tb, const Img out,          \
                                                      uint32_t start, uint32_t end) {                                    \
        module_spans<ZF, A>(a, tb, out, start, end);                                                                     \
    }
// a per-sub-span value of one field: the span array's entry, or the value the field has without one
__device__ __forceinline__ float span_f(const float *arr, size_t kv, float dflt) { return arr ? arr[kv] : dflt; }
__device__ __forceinline__ uint32_t span_u(const uint32_t *arr, size_t kv, uint32_t dflt) { return arr ? arr[kv] : dflt; }

// ---- host side of the span paints (zh_<m>_paint_spans)
enum { SPAN_F = 1, SPAN_U = 2 };   // which arrays a field takes
static inline bool module_span_table_ok(const zh_script_span_table *t) {
    return t && t->max_spans > 0 && t->count && t->start && t->end && t->note_id_changed;
}
static inline SpanWalkP mk_span_walk(const zh_script_span_table *t) {
    return SpanWalkP{t->max_spans, t->count, t->start, t->end, t->note_id_changed};
}
static inline bool note_span_table_ok(const zh_span_table *t) {
    return t && t->max_spans > 0 && t->count && t->start && t->end && t->freq && t->note_on && t->note_id_changed;
}
static inline NoteSpanTableP mk_note_span_table(const zh_span_table *t) {
    return NoteSpanTableP{t->max_spans, t->count, t->start, t->end, t->freq, t->note_on, t->note_id_changed};
}
// every array of span_params (NULL = none) on a field that takes it
static inline bool module_span_params_ok(const zh_script_span_param *sp, const uint8_t *kinds, int n) {
    if (!sp) return true;
    for (int i = 0; i < n; i++)
        if ((sp[i].f && !(kinds[i] & SPAN_F)) || (sp[i].u && !(kinds[i] & SPAN_U))) return false;
    return true;
}
static inline const float *span_fa(const zh_script_span_param *sp, int i) { return sp ? sp[i].f : nullptr; }
static inline const uint32_t *span_ua(const zh_script_span_param *sp, int i) { return sp ? sp[i].u : nullptr; }
static inline bool span_has(const zh_script_span_param *sp, int i) { return sp && (sp[i].f || sp[i].u); }
// launch NAME<zf, ADAPTER...> over the module's voices (zf, st, a, m, table, outputs, start, end in scope)
#define ZH_MODULE_SPANS_LAUNCH(NAME, ...)                                                                                  \
    do {                                                                                                                  \
        if (zf) ZH_LAUNCH((NAME<true, __VA_ARGS__>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, mk_span_walk(table),      \
                          mk_img(outputs[0]), start, end);                                                                \
        else ZH_LAUNCH((NAME<false, __VA_ARGS__>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, mk_span_walk(table),        \
                       mk_img(outputs[0]), start, end);                                                                   \
    } while (0)
#endif
