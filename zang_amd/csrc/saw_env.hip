// saw_env.hip -- InnerInstrument.paint (examples/example_subsong.zig:43-67) as ONE fused kernel per paint:
//   k_saw_env_spans<ZF, TB>   the Trigger loop of SubtrackPlayer.paint (:135-143) for every voice from a span table
// in the shape of k_lead_spans (lead.hip) and k_hard_square_spans: a lane per voice, contraction off, the state loaded and stored
// once, span_walk's segments, one read-modify-write column.  The plain paint is the same kernel over a table of one sub-span per
// voice that holds no arrays (lead.hip.h LeadOneSpanP).  Not built: a few-voice or frame-parallel form.
#include "common.hip.h"
#include "span_walk.hip.h"
#include "saw_env.hip.h"
#include <vector>

struct zh_saw_env {
    zh_ctx *ctx;
    uint32_t n;
    uint32_t *state;                     // [kSawEnvState][n]
};

typedef LeadArgs<zh_saw_env_patch> SawEnvArgs;

// Idle lanes of the last wave shadow voice 0 read-only and store nothing.
template <bool ZF, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_saw_env_spans(const SawEnvArgs a, const TB tb, const Img out, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    SawEnvLane n;
    n.load_state(a.state, a.V, v);
    const float freq0 = a.freq.get(v);
    const uint32_t note_on0 = a.note_on.get(v) ? 1u : 0u;
    const Img none{nullptr, 0};
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { n.begin(a, span_f(a.sf, kv, freq0), span_u(a.sn, kv, note_on0) != 0, nic); },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA { if (live) lead_paint_frames<ZF, false>(n, out, none, v, f0, f1, active); },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}
static int se_args(zh_saw_env *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_saw_env_params *p,
                   const zh_script_span_param *sp, SawEnvArgs &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    a = SawEnvArgs{m->n, m->state, p->sample_rate, p->patch, mk_f32(p->freq), mk_bool(p->note_on),
                   span_fa(sp, ZH_SAW_ENV_SPAN_FREQ), span_ua(sp, ZH_SAW_ENV_SPAN_NOTE_ON)};
    return ZH_OK;
}

template <class TB>
static void se_launch(zh_saw_env *m, const SawEnvArgs &a, const TB &tb, const zh_buf *outputs, uint32_t start, uint32_t end, uint32_t flags) {
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]);
    if (flags & ZH_PAINT_ZERO_FIRST) ZH_LAUNCH((k_saw_env_spans<true, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, start, end);
    else ZH_LAUNCH((k_saw_env_spans<false, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, start, end);
}

extern "C" {

int zh_saw_env_patch_default(zh_saw_env_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_saw_env_patch{0.0f, 0.025f, 0.1f, 0.15f, 0.5f};            // :55, :60-63
    return ZH_OK;
}
int zh_saw_env_create(zh_ctx *ctx, uint32_t n, zh_saw_env **out) { ZH_GUARD(ctx);
    if (!ctx || !out) return ZH_ERR_INVALID;
    zh_saw_env *m = new (std::nothrow) zh_saw_env();
    if (!m) return ZH_ERR_INVALID;
    m->ctx = ctx; m->n = n; m->state = nullptr;
    int rc = dev_alloc(&m->state, (size_t)kSawEnvState * n);            // init() :36-41: every word zero (idle is 0)
    if (!rc && n) { hipError_t e = hipMemsetAsync(m->state, 0, (size_t)kSawEnvState * n * 4, ctx->stream); if (e != hipSuccess) rc = (int)e; }
    if (rc) { (void)hipFree(m->state); delete m; return rc; }
    *out = m;
    return ZH_OK;
}
int zh_saw_env_destroy(zh_saw_env *m) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    (void)hipFree(m->state);
    delete m;
    return ZH_OK;
}
int zh_saw_env_get_state(zh_saw_env *m, zh_saw_env_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)kSawEnvState * n);
    int rc = zh_download(m->ctx, w.data(), m->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < n; v++) se_unpack(host[v], w.data(), n, v);
    return ZH_OK;
}
int zh_saw_env_set_state(zh_saw_env *m, const zh_saw_env_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m || !host) return ZH_ERR_INVALID;
    const size_t n = m->n;
    std::vector<uint32_t> w((size_t)kSawEnvState * n);
    for (size_t v = 0; v < n; v++) se_pack(host[v], w.data(), n, v);
    return n ? zh_upload(m->ctx, m->state, w.data(), w.size() * 4) : ZH_OK;
}
int zh_saw_env_paint(zh_saw_env *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                     const zh_saw_env_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    SawEnvArgs a;
    int rc = se_args(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    const LeadOneSpanP tb{1, {1}, {start}, {end}, {mk_bool(note_id_changed)}};
    se_launch(m, a, tb, outputs, start, end, flags);
    return zh_launch_status();
}
int zh_saw_env_paint_spans(zh_saw_env *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps,
                           const zh_saw_env_params *p, const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) {
    ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    static const uint8_t kinds[ZH_SAW_ENV_SPAN_FIELDS] = {SPAN_F, SPAN_U};
    SawEnvArgs a;
    int rc = se_args(m, start, end, outputs, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, kinds, ZH_SAW_ENV_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    se_launch(m, a, mk_span_walk(table), outputs, start, end, flags);
    return zh_launch_status();
}

}  // extern "C"
