// hard_square.hip -- HardSquareInstrument.paint (examples/modules.zig:269-288) plus the addScalarInto of
// examples/example_arpeggiator.zig:115 as ONE fused kernel per paint:
//   k_hard_square_spans<ZF, O1, TB>   the Trigger loop of Arpeggiator.paint (:106-116) for every voice from a span table
// in the shape of k_lead_spans (lead.hip): a lane per voice, contraction off, the PulseOsc's cnt loaded and stored once,
// span_walk's segments, two read-modify-write columns (the audio image and, O1, the frequency image).  The plain paint is the same
// kernel over a table of one sub-span per voice that holds no arrays.  Not built: a few-voice or frame-parallel form.
#include "common.hip.h"
#include "span_walk.hip.h"
#include "hard_square.hip.h"
#include <vector>

struct zh_hard_square {
    zh_ctx *ctx;
    uint32_t n;
    uint32_t *state;                     // [kHardSquareState][n]
};

typedef LeadArgs<HardSquarePatch> HardSquareArgs;

// Idle lanes of the last wave shadow voice 0 read-only and store nothing.
template <bool ZF, bool O1, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_hard_square_spans(const HardSquareArgs a, const TB tb, const Img out, const Img out1, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    HardSquareLane n;
    n.load_state(a.state, a.V, v);
    const float freq0 = a.freq.get(v);
    const uint32_t note_on0 = a.note_on.get(v) ? 1u : 0u;
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { n.begin(a, span_f(a.sf, kv, freq0), span_u(a.sn, kv, note_on0) != 0, nic); },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA { if (live) lead_paint_frames<ZF, O1>(n, out, out1, v, f0, f1, active); },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}
// every voice has ONE sub-span, the span itself: a table that holds no arrays (note_id_changed reaches no module)
struct HardSquareOneSpanP {
    struct U32 { uint32_t x; __device__ __forceinline__ uint32_t operator[](size_t) const { return x; } };
    uint32_t K;
    U32 count, start, end, nic;
};

static int hs_args(zh_hard_square *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_hard_square_params *p,
                   const zh_script_span_param *sp, HardSquareArgs &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    if (outputs[1].ptr && !buf_covers(outputs[1], m->n, end)) return ZH_ERR_INVALID;
    a = HardSquareArgs{m->n, m->state, p->sample_rate, HardSquarePatch{}, mk_f32(p->freq), mk_bool(p->note_on),
                       span_fa(sp, ZH_HARD_SQUARE_SPAN_FREQ), span_ua(sp, ZH_HARD_SQUARE_SPAN_NOTE_ON)};
    return ZH_OK;
}

template <class TB>
static void hs_launch(zh_hard_square *m, const HardSquareArgs &a, const TB &tb, const zh_buf *outputs, uint32_t start, uint32_t end, uint32_t flags) {
    const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0, o1 = outputs[1].ptr != nullptr;
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]), out1 = o1 ? mk_img(outputs[1]) : Img{nullptr, 0};
    if (zf && o1) ZH_LAUNCH((k_hard_square_spans<true, true, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
    else if (zf) ZH_LAUNCH((k_hard_square_spans<true, false, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
    else if (o1) ZH_LAUNCH((k_hard_square_spans<false, true, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
    else ZH_LAUNCH((k_hard_square_spans<false, false, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, out1, start, end);
}

extern "C" {

int zh_hard_square_create(zh_ctx *ctx, uint32_t n, zh_hard_square **out) { ZH_GUARD(ctx);
    if (!ctx || !out) return ZH_ERR_INVALID;
    zh_hard_square *m = new (std::nothrow) zh_hard_square();
    if (!m) return ZH_ERR_INVALID;
    m->ctx = ctx; m->n = n; m->state = nullptr;
    int rc = dev_alloc(&m->state, (size_t)kHardSquareState * n);        // init(): PulseOsc.init's cnt = 0 (modules.zig:262-267)
    if (!rc && n) { hipError_t e = hipMemsetAsync(m->state, 0, (size_t)kHardSquareState * n * 4, ctx->stream); if (e != hipSuccess) rc = (int)e; }
    if (rc) { (void)hipFree(m->state); delete m; return rc; }
    *out = m;
    return ZH_OK;
}
int zh_hard_square_destroy(zh_hard_square *m) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->state);
    delete m;
    return ZH_OK;
}
int zh_hard_square_get_state(zh_hard_square *m, zh_hard_square_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)kHardSquareState * n);
    int rc = zh_download(m->ctx, w.data(), m->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < n; v++) hs_unpack(host[v], w.data(), n, v);
    return ZH_OK;
}
int zh_hard_square_set_state(zh_hard_square *m, const zh_hard_square_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)kHardSquareState * n);
    for (size_t v = 0; v < n; v++) hs_pack(host[v], w.data(), n, v);
    return n ? zh_upload(m->ctx, m->state, w.data(), w.size() * 4) : ZH_OK;
}
int zh_hard_square_paint(zh_hard_square *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                         const zh_hard_square_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps; (void)note_id_changed;
    HardSquareArgs a;
    int rc = hs_args(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    const HardSquareOneSpanP tb{1, {1}, {start}, {end}, {0}};
    hs_launch(m, a, tb, outputs, start, end, flags);
    return zh_launch_status();
}
int zh_hard_square_paint_spans(zh_hard_square *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps,
                               const zh_hard_square_params *p, const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) {
    ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    static const uint8_t kinds[ZH_HARD_SQUARE_SPAN_FIELDS] = {SPAN_F, SPAN_U};
    HardSquareArgs a;
    int rc = hs_args(m, start, end, outputs, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, kinds, ZH_HARD_SQUARE_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    hs_launch(m, a, mk_span_walk(table), outputs, start, end, flags);
    return zh_launch_status();
}

}  // extern "C"
