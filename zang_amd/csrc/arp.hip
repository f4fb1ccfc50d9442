// arp.hip -- the arpeggiator stage: Arpeggiator.paint of examples/example_arpeggiator.zig (:49-117) without its instrument, for
// n players on the device.  k_arp_schedule, one lane per player, reads the sub-span table a live voice bank of polyphony 1 filled
// from the held-key records (MainModule.paint :153-156) and writes the stage's own [span][player] table, which the span paints
// read in place.  The per-lane steps are arp_lane.hip.h; semantics and what is defined where the reference is not: zang_hip.h.
#include "common.hip.h"
#include "arp_lane.hip.h"
#include <vector>
#include <string.h>

namespace {
constexpr uint32_t kArpBlock = 64;
constexpr uint32_t kArpDefaultRows = 4;

struct ArpArgs {
    uint32_t n, n_keys, nd, out_len, in_spans, max_spans;
    const uint32_t *key_freq_bits;                                    // [n_keys]
    const uint32_t *in_count, *in_start, *in_end, *held_lo, *held_hi; // the outer table, [in_spans][n]
    uint32_t *state;                                                  // [kArpState][n]
    uint32_t *count, *start, *end, *freq, *note_on;                   // the stage's table, [rows][n]
    uint8_t *changed;
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kArpBlock) k_arp_schedule(const ArpArgs a) {
    const uint32_t p = blockIdx.x * kArpBlock + threadIdx.x;
    if (p >= a.n) return;
    const size_t n = a.n;
    ArpLane s;
    arp_load(s, a.state, n, p);
    const uint32_t cnt = min(a.in_count[p], a.in_spans);
    uint32_t k = 0, dropped = 0;
    arp_buffer(s, a.key_freq_bits, a.n_keys, a.nd, a.out_len, cnt, a.in_start + p, a.in_end + p, a.held_lo + p, a.held_hi + p, n,
               [&](uint32_t s0, uint32_t s1, uint32_t freq_bits, uint32_t note_on, uint32_t changed) {
        if (k >= a.max_spans) { dropped++; return; }
        const size_t idx = (size_t)k * n + p;
        a.start[idx] = s0; a.end[idx] = s1; a.freq[idx] = freq_bits; a.note_on[idx] = note_on; a.changed[idx] = (uint8_t)changed;
        k++;
    });
    a.count[p] = k;
    arp_store(s, a.state, n, p);
    if (dropped) atomicAdd(a.overflow, dropped);
}
}  // namespace

struct zh_arp {
    zh_ctx *ctx;
    uint32_t n, n_keys, rows;
    uint32_t *key_freq_bits, *state;
    uint32_t *count, *start, *end, *freq, *note_on;
    uint8_t *changed;
    uint32_t *overflow;
};

namespace {
void arp_free_tables(zh_arp *a) {
    (void)hipFree(a->start); (void)hipFree(a->end); (void)hipFree(a->freq); (void)hipFree(a->note_on); (void)hipFree(a->changed);
    a->start = a->end = a->freq = a->note_on = nullptr; a->changed = nullptr; a->rows = 0;
}
void arp_free(zh_arp *a) {
    arp_free_tables(a);
    (void)hipFree(a->key_freq_bits); (void)hipFree(a->state); (void)hipFree(a->count); (void)hipFree(a->overflow);
}
int arp_alloc_tables(zh_arp *a, uint32_t rows) {
    const size_t cells = (size_t)rows * a->n;
    int rc = dev_alloc(&a->start, cells);
    if (!rc) rc = dev_alloc(&a->end, cells);
    if (!rc) rc = dev_alloc(&a->freq, cells);
    if (!rc) rc = dev_alloc(&a->note_on, cells);
    if (!rc) rc = dev_alloc(&a->changed, cells);
    if (rc) { arp_free_tables(a); (void)hipGetLastError(); return rc; }
    a->rows = rows;
    return ZH_OK;
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
    if (!rc) rc = dev_alloc(&a->count, (size_t)n_players);
    if (!rc) rc = dev_alloc(&a->overflow, 1);
    if (!rc) rc = arp_alloc_tables(a, kArpDefaultRows);
    if (!rc) rc = (int)hipMemsetAsync(a->overflow, 0, 4, ctx->stream);
    if (!rc && n_players) rc = (int)hipMemsetAsync(a->count, 0, (size_t)n_players * 4, ctx->stream);
    if (!rc) rc = zh_upload(ctx, a->key_freq_bits, key_freqs, (size_t)n_keys * 4);
    if (!rc) rc = arp_upload_init(a);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); arp_free(a); delete a; (void)hipGetLastError(); return rc; }
    *out = a;
    return ZH_OK;
}

int zh_arp_destroy(zh_arp *a) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a) return ZH_ERR_INVALID;
    if (!a->ctx->capturing) (void)hipStreamSynchronize(a->ctx->stream);
    arp_free(a);
    delete a;
    return ZH_OK;
}

int zh_arp_reset(zh_arp *a) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a) return ZH_ERR_INVALID;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;                 // the upload reads host memory
    return arp_upload_init(a);
}

int zh_arp_reserve(zh_arp *a, uint32_t max_rows) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || max_rows == 0) return ZH_ERR_INVALID;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    if (max_rows == a->rows) return ZH_OK;
    ZH_TRY(hipStreamSynchronize(a->ctx->stream));
    arp_free_tables(a);
    return arp_alloc_tables(a, max_rows);
}

int zh_arp_schedule(zh_arp *a, float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in,
                    const zh_script_span_param *held) { ZH_GUARD(a ? a->ctx : nullptr);
    uint32_t nd = 0;
    if (!a || !in || !held || max_spans == 0 || max_spans > a->rows || in->max_spans == 0 || !in->count || !in->start || !in->end ||
        !held[0].u || !held[1].u || !arp_note_duration(sample_rate, nd))
        return ZH_ERR_INVALID;
    if (a->n == 0) return ZH_OK;
    const ArpArgs args{a->n, a->n_keys, nd, out_len, in->max_spans, max_spans, a->key_freq_bits, in->count, in->start, in->end,
                       held[0].u, held[1].u, a->state, a->count, a->start, a->end, a->freq, a->note_on, a->changed, a->overflow};
    ZH_LAUNCH(k_arp_schedule, dim3((a->n + kArpBlock - 1) / kArpBlock), dim3(kArpBlock), 0, a->ctx->stream, args);
    return zh_launch_status();
}

int zh_arp_script_table(const zh_arp *a, uint32_t max_spans, zh_script_span_table *out) {
    if (!a || !out || max_spans == 0 || max_spans > a->rows) return ZH_ERR_INVALID;
    *out = zh_script_span_table{max_spans, 0, a->count, a->start, a->end, a->changed};
    return ZH_OK;
}
int zh_arp_span_param(const zh_arp *a, uint32_t field, zh_script_span_param *out) {
    if (!a || !out || field >= ZH_ARP_SPAN_FIELDS) return ZH_ERR_INVALID;
    *out = field == ZH_ARP_SPAN_FREQ ? zh_script_span_param{(const float *)a->freq, nullptr} : zh_script_span_param{nullptr, a->note_on};
    return ZH_OK;
}

int zh_arp_overflows(zh_arp *a, uint64_t *out) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || !out) return ZH_ERR_INVALID;
    uint32_t w = 0;
    int rc = zh_download(a->ctx, &w, a->overflow, 4);
    *out = w;
    return rc;
}

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
