// arp.hip -- the arpeggiator stage: Arpeggiator.paint of examples/example_arpeggiator.zig (:49-117) without its instrument, for
// n players on the device.  k_arp_schedule, one lane per player, reads the sub-span table a live voice bank of polyphony 1 filled
// from the held-key records (MainModule.paint :153-156) and writes the stage's own [span][player] table, which the span paints
// read in place.  The per-lane steps are arp_lane.hip.h; semantics and what is defined where the reference is not: zang_hip.h.
#include "common.hip.h"
#include "arp_lane.hip.h"
#include "span_stage.hip.h"
#include <vector>
#include <string.h>

namespace {
constexpr uint32_t kArpBlock = 64;
constexpr uint32_t kArpDefaultRows = 4;
static_assert(ZH_ARP_SPAN_FREQ == 0 && ZH_ARP_SPAN_NOTE_ON == 1 && ZH_ARP_SPAN_FIELDS == 2, "the fields StageWriter emits");

struct ArpArgs {
    uint32_t n, n_keys, nd, out_len, in_spans, max_spans;
    const uint32_t *key_freq_bits;                                    // [n_keys]
    const uint32_t *in_count, *in_start, *in_end, *held_lo, *held_hi; // the outer table, [in_spans][n]
    uint32_t *state;                                                  // [kArpState][n]
    StageRows out;                                                    // the stage's table: fields ZH_ARP_SPAN_FREQ, _NOTE_ON
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kArpBlock) k_arp_schedule(const ArpArgs a) {
    const uint32_t p = blockIdx.x * kArpBlock + threadIdx.x;
    if (p >= a.n) return;
    const size_t n = a.n;
    ArpLane s;
    arp_load(s, a.state, n, p);
    const uint32_t cnt = min(a.in_count[p], a.in_spans);
    StageWriter emit{a.out, n, p, a.max_spans, 0, 0};
    arp_buffer(s, a.key_freq_bits, a.n_keys, a.nd, a.out_len, cnt, a.in_start + p, a.in_end + p, a.held_lo + p, a.held_hi + p, n, emit);
    a.out.count[p] = emit.k;
    arp_store(s, a.state, n, p);
    if (emit.dropped) atomicAdd(a.overflow, emit.dropped);
}
}  // namespace

struct zh_arp : zh_stage {
    uint32_t n, n_keys;
    uint32_t *key_freq_bits, *state;
};

namespace {
void arp_free(zh_arp *a) {
    stage_free(a->tab);
    (void)hipFree(a->key_freq_bits); (void)hipFree(a->state);
}
void arp_pack(const zh_arp_state &h, uint32_t *w, size_t n, size_t v) {
    uint32_t fb;
    memcpy(&fb, &h.freq, 4);
    arp_store(ArpLane{h.next_frame, h.next_id, h.last_note, h.has_note, h.note_id, fb, h.note_on}, w, n, v);
}
int arp_upload_init(zh_arp *a) {                                      // init() :38-47
    if (!a->n) return ZH_OK;
    std::vector<uint32_t> w((size_t)kArpState * a->n);
    ArpLane s;
    arp_init(s);
    for (size_t v = 0; v < a->n; v++) arp_store(s, w.data(), a->n, v);
    return zh_upload(a->ctx, a->state, w.data(), w.size() * 4);
}
}  // namespace

extern "C" {

int zh_arp_create(zh_ctx *ctx, uint32_t n_players, const float *key_freqs, uint32_t n_keys, zh_arp **out) { ZH_GUARD(ctx);
    if (!ctx || !out || !key_freqs || n_keys == 0 || n_keys > kArpMaxKeys || n_players > (1u << 31)) return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    zh_arp *a = new (std::nothrow) zh_arp();
    if (!a) return ZH_ERR_INVALID;
    memset(a, 0, sizeof *a);
    a->ctx = ctx; a->n = n_players; a->n_keys = n_keys;
    int rc = dev_alloc(&a->key_freq_bits, (size_t)n_keys);
    if (!rc) rc = dev_alloc(&a->state, (size_t)kArpState * n_players);
    if (!rc) rc = stage_create(a, n_players, ZH_ARP_SPAN_FIELDS, kArpDefaultRows);
    if (!rc) rc = zh_upload(ctx, a->key_freq_bits, key_freqs, (size_t)n_keys * 4);
    if (!rc) rc = arp_upload_init(a);
    if (rc) return stage_create_failed(a, arp_free, rc);
    *out = a;
    return ZH_OK;
}

int zh_arp_destroy(zh_arp *a) { ZH_GUARD(a ? a->ctx : nullptr); return stage_destroy(a, arp_free); }

int zh_arp_reset(zh_arp *a) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a) return ZH_ERR_INVALID;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;                 // the upload reads host memory
    return arp_upload_init(a);
}

int zh_arp_reserve(zh_arp *a, uint32_t max_rows) { ZH_GUARD(a ? a->ctx : nullptr); return stage_reserve(a, max_rows); }

int zh_arp_schedule(zh_arp *a, float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in,
                    const zh_script_span_param *held) { ZH_GUARD(a ? a->ctx : nullptr);
    uint32_t nd = 0;
    if (!stage_spans_ok(a, max_spans) || !stage_input_ok(in, false) || !held || !held[0].u || !held[1].u || !arp_note_duration(sample_rate, nd))
        return ZH_ERR_INVALID;
    if (a->n == 0) return ZH_OK;
    const ArpArgs args{a->n, a->n_keys, nd, out_len, in->max_spans, max_spans, a->key_freq_bits, in->count, in->start, in->end,
                       held[0].u, held[1].u, a->state, stage_rows(a), a->tab.overflow};
    ZH_LAUNCH(k_arp_schedule, dim3((a->n + kArpBlock - 1) / kArpBlock), dim3(kArpBlock), 0, a->ctx->stream, args);
    return zh_launch_status();
}

int zh_arp_script_table(const zh_arp *a, uint32_t max_spans, zh_script_span_table *out) { return stage_script_table(a, max_spans, out); }
int zh_arp_span_param(const zh_arp *a, uint32_t field, zh_script_span_param *out) {
    return stage_span_param(a, field, field == ZH_ARP_SPAN_FREQ ? 'f' : 'u', out);
}
int zh_arp_overflows(zh_arp *a, uint64_t *out) { ZH_GUARD(a ? a->ctx : nullptr); return stage_overflows(a, out); }

int zh_arp_get_state(zh_arp *a, zh_arp_state *host) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || (a->n && !host)) return ZH_ERR_INVALID;
    if (!a->n) return ZH_OK;
    std::vector<uint32_t> w((size_t)kArpState * a->n);
    int rc = zh_download(a->ctx, w.data(), a->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < a->n; v++) {
        ArpLane s;
        arp_load(s, w.data(), a->n, v);
        zh_arp_state h{s.next_frame, s.next_id, s.last_note, s.has_note, s.note_id, 0.0f, s.note_on};
        memcpy(&h.freq, &s.freq_bits, 4);
        host[v] = h;
    }
    return ZH_OK;
}
int zh_arp_set_state(zh_arp *a, const zh_arp_state *host) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || (a->n && !host)) return ZH_ERR_INVALID;
    if (!a->n) return ZH_OK;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    std::vector<uint32_t> w((size_t)kArpState * a->n);
    for (size_t v = 0; v < a->n; v++) {
        if (host[v].last_note < -1 || host[v].last_note >= (int32_t)a->n_keys) return ZH_ERR_INVALID;   // it indexes the key table
        arp_pack(host[v], w.data(), a->n, v);
    }
    return zh_upload(a->ctx, a->state, w.data(), w.size() * 4);
}

}  // extern "C"
