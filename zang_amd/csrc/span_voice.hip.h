// span_voice.hip.h -- what the fused voices that paint one LANE per voice from a span table share (lead.hip, hard_square.hip,
// saw_env.hip, detuned.hip; laser.hip takes the host side alone, curve_player.hip all but the kernel's body).  Two parts, both
// hipcc only (what a state Layout is made of, the plain C++ the stand-alone harnesses of tests/cpp include, and the block-level
// get / set: state_block.hip.h, which this header includes):
//   the device side: the frame loop over one or two columns, and ZH_SPAN_VOICE_KERNEL, the kernel on span_walk's segments under
//   each voice's stable kernel name;
//   the host side: the handle {ctx, n, state} with create / destroy / get_state / set_state over a Layout (PortaLayout,
//   VibratoLayout, HardSquareLayout, SawEnvLayout, DetunedLayout, LaserLayout, CurvePlayerLayout, ...), the zf x o1 launch switch,
//   and the two paint entry points.
// A voice's translation unit is then its handle type, one ZH_SPAN_VOICE_KERNEL line, patch_default and the extern "C" wrappers.
#pragma once
#include "state_block.hip.h"

#if defined(__HIPCC__)
#include "common.hip.h"
#include "seq.hip.h"
#include "span_walk.hip.h"
#include <new>
#include <vector>

// ---- the device side ---------------------------------------------------------------------------------------------------
// A lane L:
//   L::Args                              the kernel's argument block: a.V = voices, a.state = [words][V].  The per-sub-span fields are
//                                        its business: Args::Span, a.defaults(v) = the fields of a sub-span without span arrays,
//                                        a.span(kv, defaults) = those of sub-span kv
//   L::kOutputs                          columns painted: 1, or 2 (outputs[1] may then be absent, O1 = false)
//   load_state(st, V, v) / store_state   the voice's words; load_state also gives every field begin() sets a value
//   begin(a, span, nic)                  the prologue of the voice's paint(), at every sub-span
//   frame(f) -> what is added to outputs[0], f = what is added to outputs[1]
//   end()                                its epilogue

// frames [f0, f1) of one voice; `active` = false paints nothing.  outputs[0] goes through frame_loop, input-free.  The second
// column (O1): a ZERO_FIRST paint stores it frame by frame; an ADD paint hands the image to frame_loop as an INPUT, so that its
// rows are fetched a chunk ahead like the output's, and stores old + f -- frame_loop reads the rows of chunk k + 1 before chunk k
// is computed and a frame's own row before its body in the tail: a row is never read after it was written.  Inside a sub-span
// EVERY frame of both columns is added to, a +-0.0 addend included.
template <bool ZF, bool O1, class L>
__device__ __forceinline__ void span_voice_frames(L &n, const Img &out, const Img &out1, uint32_t v, uint32_t f0, uint32_t f1, bool active) {
    constexpr int NIN = (O1 && !ZF) ? 1 : 0;
    const float *ins[1] = {out1.p};
    const size_t istr[1] = {out1.stride};
    const uint32_t voff = v * 4u;
    frame_loop<8, ZF, NIN>(out.p, v, out.stride, ins, istr, f0, f1, [&](uint32_t i, const float (&x)[1], float &val) ZH_INLINE_LAMBDA {
        float f = 0.0f;
        if (active) val = n.frame(f);
        if constexpr (O1) {
            if (ZF) zrow_store<1>(zrow_rsrc(out1.p, out1.stride, i), voff, 0, active ? 0.0f + f : 0.0f);
            else if (active) zrow_store<1>(zrow_rsrc(out1.p, out1.stride, i), voff, 0, x[0] + f);
        }
        return active;
    });
}

// One voice's span paint, one lane per voice (kSeqBlock-lane blocks over seq_grid(V)): NAME<ZF, O1, Lane, TB> under its stable
// kernel name (zh_last_form, zh_graph_kernels, rocprofv3), and NAME_launch, which hands that name to the host side below.  TB:
// SpanWalkP, or OneSpanP (the plain paints).  Idle lanes of the last wave shadow voice 0 read-only and store nothing.  The voice's
// words are loaded and stored once; the fields of a sub-span without span arrays are read once, before the walk.
// (The body stands in the kernel itself: behind a __device__ function, as span_walk.hip.h module_spans, the same instructions came
// out in another order and in other registers in every instantiation.)
#define ZH_SPAN_VOICE_KERNEL(NAME)                                                                                         \
    template <bool ZF, bool O1, class L, class TB>                                                                        \
    __global__ void __launch_bounds__(kSeqBlock) NAME(const typename L::Args a, const TB tb, const Img out, const Img out1, \
                                                      uint32_t start, uint32_t end) {                                    \
        const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;                                                         \
        const bool live = v0 < a.V;                                                                                       \
        const uint32_t v = live ? v0 : 0;                                                                                 \
        L n;                                                                                                              \
        n.load_state(a.state, a.V, v);                                                                                    \
        const typename L::Args::Span d = a.defaults(v);                                                                   \
        span_walk_segments(tb, a.V, v, live, start, end,                                                                  \
                           [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { n.begin(a, a.span(kv, d), nic); },                 \
                           [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA {                                  \
                               if (live) span_voice_frames<ZF, O1>(n, out, out1, v, f0, f1, active);                      \
                           },                                                                                             \
                           [&]() ZH_INLINE_LAMBDA { n.end(); });                                                          \
        if (live) n.store_state(a.state, a.V, v);                                                                         \
    }                                                                                                                     \
    ZH_VOICE_LAUNCHER(NAME, (NAME<ZF, O1, L, TB>))
// NAME_launch::go<ZF, O1, L, TB>(...) launches KERNEL, an instantiation that starts with NAME (ZH_LAUNCH records that token)
#define ZH_VOICE_LAUNCHER(NAME, KERNEL)                                                                                    \
    struct NAME##_launch {                                                                                                \
        template <bool ZF, bool O1, class L, class TB>                                                                    \
        static void go(dim3 grid, hipStream_t st, const typename L::Args &a, const TB &tb, const Img &out, const Img &out1, \
                       uint32_t start, uint32_t end) {                                                                   \
            ZH_LAUNCH(KERNEL, grid, dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);                                \
        }                                                                                                                 \
    };

// ---- the host side -----------------------------------------------------------------------------------------------------
// the base of the voices' opaque handles (zh_porta, zh_vibrato, zh_hard_square, zh_saw_env, zh_detuned, zh_laser, zh_curve_player)
struct zh_voice {
    zh_ctx *ctx;
    uint32_t n;
    uint32_t *state;                     // [Layout::kWords][n]
};

// init(): every word zero
template <class M> static int voice_create(zh_ctx *ctx, uint32_t n, uint32_t words, M **out) {
    if (!ctx || !out) return ZH_ERR_INVALID;
    M *m = new (std::nothrow) M();
    if (!m) return ZH_ERR_INVALID;
    m->ctx = ctx; m->n = n;
    int rc = dev_alloc_zeroed(ctx, &m->state, (size_t)words * n);
    if (rc) { (void)hipFree(m->state); delete m; return rc; }
    *out = m;
    return ZH_OK;
}
template <class M> static int voice_destroy(M *m) {
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->state);
    delete m;
    return ZH_OK;
}
template <class LY> static int voice_get_state(zh_voice *m, typename LY::State *host) {
    return m && host ? block_get_state<LY>(m->ctx, m->state, m->n, host) : ZH_ERR_INVALID;
}
template <class LY> static int voice_set_state(zh_voice *m, const typename LY::State *host) {
    return m && host ? block_set_state<LY>(m->ctx, m->state, m->n, host) : ZH_ERR_INVALID;
}

// The paints of a lane L that also names
//   L::Params, L::args(m, p, sp) -> Args   the ABI's parameter record and the kernel's arguments from it (sp: the span arrays, or NULL)
//   L::kinds[L::kFields]                   which arrays each span field takes (SPAN_F / SPAN_U)
// K: the kernel's NAME_launch.

// what both paints check first, and the kernel's arguments.  outputs[] has L::kOutputs entries: a one-column voice's has no [1].
template <class L>
static int voice_args(zh_voice *m, uint32_t start, uint32_t end, const zh_buf *outputs, const typename L::Params *p, const zh_script_span_param *sp,
                      typename L::Args &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    // (the two columns are painted in one pass, each frame of outputs[1] after that of outputs[0]: they may not share a float)
    if constexpr (L::kOutputs > 1) {
        if (outputs[1].ptr && (!buf_covers(outputs[1], m->n, end) || views_overlap(outputs[0], outputs[1], m->n))) return ZH_ERR_INVALID;
    }
    a = L::args(*m, *p, sp);
    return ZH_OK;
}
// K<zf, o1, L, TB> over the module's voices; o1 = outputs[1] is painted
template <class K, class L, class TB>
static void voice_launch(zh_voice *m, const typename L::Args &a, const TB &tb, const zh_buf *outputs, uint32_t start, uint32_t end, uint32_t flags) {
    const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0;
    const dim3 grid = seq_grid(m->n);
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]);
    if constexpr (L::kOutputs > 1) {
        if (outputs[1].ptr) {
            const Img out1 = mk_img(outputs[1]);
            if (zf) K::template go<true, true, L>(grid, st, a, tb, out, out1, start, end);
            else K::template go<false, true, L>(grid, st, a, tb, out, out1, start, end);
            return;
        }
    }
    const Img none{nullptr, 0};
    if (zf) K::template go<true, false, L>(grid, st, a, tb, out, none, start, end);
    else K::template go<false, false, L>(grid, st, a, tb, out, none, start, end);
}
// zh_<voice>_paint: the same kernel over the table of one sub-span per voice
template <class K, class L>
static int voice_paint(zh_voice *m, uint32_t start, uint32_t end, const zh_buf *outputs, BoolP note_id_changed, const typename L::Params *p, uint32_t flags) {
    typename L::Args a;
    int rc = voice_args<L>(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    voice_launch<K, L>(m, a, OneSpanP{1, {1}, {start}, {end}, {note_id_changed}}, outputs, start, end, flags);
    return zh_launch_status();
}
template <class K, class L>
static int voice_paint_spans(zh_voice *m, uint32_t start, uint32_t end, const zh_buf *outputs, const typename L::Params *p, const zh_script_span_param *sp,
                             const zh_script_span_table *table, uint32_t flags) {
    typename L::Args a;
    int rc = voice_args<L>(m, start, end, outputs, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, L::kinds, L::kFields)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    voice_launch<K, L>(m, a, mk_span_walk(table), outputs, start, end, flags);
    return zh_launch_status();
}
#endif   // __HIPCC__
