// pmctl.hip -- the controlled phase-modulation voice of examples/example_mouse.zig as ONE fused kernel per paint:
//   k_pmctl_spans<ZF, TB>      PMOscInstrument.paint (:46-72) for every voice over a table of notes (the Trigger loop of :193-211),
//                              ratio and multiplier constants or [frame][voice] images; the plain paint is the same kernel over a
//                              table of one sub-span per voice that holds no arrays
//   k_pmctl_controlled<ZF>     the whole of MainModule.paint (:148-211): the two controls' Portamentos, each over ITS OWN table,
//                              painted into registers under the voice -- no control image is written or read
// Both are pmctl.hip.h's pmctl_voice over its three-cursor walk: a lane per voice, contraction off, the state loaded and stored
// once.  The handle and its state calls are span_voice.hip.h's.  Not built: a few-voice or frame-parallel form.
#include "pmctl.hip.h"

struct zh_pmctl : zh_voice {};

template <bool ZF, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_pmctl_spans(const PmctlArgs a, const TB tb, const Img out, uint32_t start, uint32_t end) {
    const PmctlNoTable none{0, {}, {}, {}, {}};
    pmctl_voice<ZF, false>(a, tb, none, none, out, start, end);
}
template <bool ZF>
__global__ void __launch_bounds__(kSeqBlock) k_pmctl_controlled(const PmctlArgs a, const SpanWalkP tn, const SpanWalkP tr, const SpanWalkP tm,
                                                                const Img out, uint32_t start, uint32_t end) {
    pmctl_voice<ZF, true>(a, tn, tr, tm, out, start, end);
}

namespace {
const uint8_t kPmctlKinds[ZH_PMCTL_SPAN_FIELDS] = {SPAN_F, SPAN_U};

// what the three paints check first, and the kernel's arguments without the cobs / controls.  `flags` loses ZERO_FIRST where an
// image the paint reads overlaps the output (zh_zero_first_aliased).
int pmctl_args(zh_pmctl *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_pmctl_params *p,
               const zh_script_span_param *sp, PmctlArgs &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    const bool stale = temps && temps[1].ptr;
    if (stale && !buf_covers(temps[1], m->n, end)) return ZH_ERR_INVALID;
    a = PmctlArgs{};
    a.V = m->n; a.state = m->state; a.sample_rate = p->sample_rate; a.patch = p->patch;
    a.freq = mk_f32(p->freq); a.note_on = mk_bool(p->note_on); a.relative = mk_bool(p->relative);
    a.sf = span_fa(sp, ZH_PMCTL_SPAN_FREQ); a.sn = span_ua(sp, ZH_PMCTL_SPAN_NOTE_ON);
    a.stale = stale ? mk_img(temps[1]) : Img{nullptr, 0};
    return ZH_OK;
}
int pmctl_cobs(zh_pmctl *m, uint32_t end, const zh_cob *ratio, const zh_cob *mult, PmctlArgs &a) {
    if (!ratio || !mult || !cob_ok(*ratio, m->n, end) || !cob_ok(*mult, m->n, end)) return ZH_ERR_INVALID;
    a.ratio = mk_cob(*ratio); a.mult = mk_cob(*mult);
    return ZH_OK;
}
bool pmctl_control_ok(const zh_pmctl_control *c) {
    return c && module_span_table_ok(c->table) && c->value.f && !c->value.u && c->note_on.u && !c->note_on.f;
}
bool pmctl_reads_output(const zh_buf *outputs, const zh_buf *temps, const zh_cob *ratio, const zh_cob *mult) {
    return (temps && temps[1].ptr && bufs_alias(temps[1], outputs[0])) || (ratio && cob_aliases(*ratio, outputs[0])) ||
           (mult && cob_aliases(*mult, outputs[0]));
}
template <class TB>
void pmctl_launch_spans(zh_pmctl *m, const PmctlArgs &a, const TB &tb, const zh_buf *outputs, uint32_t start, uint32_t end, uint32_t flags) {
    hipStream_t st = m->ctx->stream;
    if (flags & ZH_PAINT_ZERO_FIRST) ZH_LAUNCH((k_pmctl_spans<true, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, mk_img(outputs[0]), start, end);
    else ZH_LAUNCH((k_pmctl_spans<false, TB>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, mk_img(outputs[0]), start, end);
}
}   // namespace

extern "C" {

int zh_pmctl_patch_default(zh_pmctl_patch *p) {
    if (!p) return ZH_ERR_INVALID;
    *p = zh_pmctl_patch{ZH_CURVE_LINEAR, 0.1f, 0.025f, 0.1f, 1.0f, 0.5f};   // example_mouse.zig:160, :184, :65-68
    return ZH_OK;
}
// init() :39-44, :123-134: every word zero (idle is 0)
int zh_pmctl_create(zh_ctx *ctx, uint32_t n, zh_pmctl **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kPmctlState, out); }
int zh_pmctl_destroy(zh_pmctl *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_pmctl_get_state(zh_pmctl *m, zh_pmctl_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<PmctlLayout>(m, host); }
int zh_pmctl_set_state(zh_pmctl *m, const zh_pmctl_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<PmctlLayout>(m, host); }

int zh_pmctl_paint(zh_pmctl *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                   const zh_pmctl_params *p, const zh_cob *ratio, const zh_cob *mult, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    PmctlArgs a;
    int rc = pmctl_args(m, start, end, outputs, temps, p, nullptr, a);
    if (!rc) rc = pmctl_cobs(m, end, ratio, mult, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    rc = zh_zero_first_aliased(m->ctx, start, end, outputs[0], m->n, pmctl_reads_output(outputs, temps, ratio, mult), flags);
    if (rc) return rc;
    pmctl_launch_spans(m, a, OneSpanP{1, {1}, {start}, {end}, {mk_bool(note_id_changed)}}, outputs, start, end, flags);
    return zh_launch_status();
}
int zh_pmctl_paint_spans(zh_pmctl *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_pmctl_params *p,
                         const zh_script_span_param *sp, const zh_script_span_table *table, const zh_cob *ratio, const zh_cob *mult,
                         uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    PmctlArgs a;
    int rc = pmctl_args(m, start, end, outputs, temps, p, sp, a);
    if (!rc) rc = pmctl_cobs(m, end, ratio, mult, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, kPmctlKinds, ZH_PMCTL_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    rc = zh_zero_first_aliased(m->ctx, start, end, outputs[0], m->n, pmctl_reads_output(outputs, temps, ratio, mult), flags);
    if (rc) return rc;
    pmctl_launch_spans(m, a, mk_span_walk(table), outputs, start, end, flags);
    return zh_launch_status();
}
int zh_pmctl_paint_controlled(zh_pmctl *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_pmctl_params *p,
                              const zh_script_span_param *sp, const zh_script_span_table *notes, const zh_pmctl_control *rc_, const zh_pmctl_control *mc_,
                              uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    PmctlArgs a;
    int rc = pmctl_args(m, start, end, outputs, temps, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(notes) || !module_span_params_ok(sp, kPmctlKinds, ZH_PMCTL_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (!pmctl_control_ok(rc_) || !pmctl_control_ok(mc_)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    rc = zh_zero_first_aliased(m->ctx, start, end, outputs[0], m->n, pmctl_reads_output(outputs, temps, nullptr, nullptr), flags);
    if (rc) return rc;
    a.rc = PmctlCtlP{rc_->value.f, rc_->note_on.u, mk_f32(rc_->scale)};
    a.mc = PmctlCtlP{mc_->value.f, mc_->note_on.u, mk_f32(mc_->scale)};
    hipStream_t st = m->ctx->stream;
    const SpanWalkP tn = mk_span_walk(notes), tr = mk_span_walk(rc_->table), tm = mk_span_walk(mc_->table);
    if (flags & ZH_PAINT_ZERO_FIRST) ZH_LAUNCH(k_pmctl_controlled<true>, seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tn, tr, tm, mk_img(outputs[0]), start, end);
    else ZH_LAUNCH(k_pmctl_controlled<false>, seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tn, tr, tm, mk_img(outputs[0]), start, end);
    return zh_launch_status();
}

}  // extern "C"
