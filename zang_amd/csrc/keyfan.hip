// keyfan.hip -- the key fan-out stage: Polyphony.paint of examples/example_polyphony.zig (:61-92) without its instruments, for n
// players of n_keys always-running voices on the device.  k_keyfan_schedule, one lane per VOICE (v = player * n_keys + key: the
// group layout of zh_mixdown_groups), reads the player's column of the sub-span table a live voice bank of polyphony 1 filled from
// the held-key records (MainModule.paint :137-145) and writes the voice's column of the stage's own [span][voice] table, which
// zh_nice_paint_spans / zh_pmosc_paint_spans (zh_keyfan_span_table) and the other span paints (zh_keyfan_script_table) read in
// place.  The per-lane steps are keyfan_lane.hip.h; semantics and what is defined where the reference is not: zang_hip.h.
#include "common.hip.h"
#include "keyfan_lane.hip.h"
#include "span_stage.hip.h"
#include <vector>
#include <string.h>

namespace {
constexpr uint32_t kKeyfanBlock = 64;
constexpr uint32_t kKeyfanDefaultRows = 4;
static_assert(ZH_KEYFAN_SPAN_FREQ == 0 && ZH_KEYFAN_SPAN_NOTE_ON == 1 && ZH_KEYFAN_SPAN_FIELDS == 2, "the fields StageWriter emits");

struct KeyfanArgs {
    uint32_t nv, n_players, n_keys, out_len, in_spans, max_spans;
    const uint32_t *key_freq_bits;                                    // [n_keys]
    const uint32_t *in_count, *in_start, *in_end, *held_lo, *held_hi; // the outer table, [in_spans][n_players]
    uint32_t *state;                                                  // [kKeyfanState][nv]
    StageRows out;                                                    // the stage's table: fields ZH_KEYFAN_SPAN_FREQ, _NOTE_ON
    uint8_t *note_on8;                                                // [rows][nv]
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kKeyfanBlock) k_keyfan_schedule(const KeyfanArgs a) {
    const uint32_t v = blockIdx.x * kKeyfanBlock + threadIdx.x;
    if (v >= a.nv) return;
    const size_t nv = a.nv, np = a.n_players;
    const uint32_t p = v / a.n_keys, key = v - p * a.n_keys;
    KeyfanLane s;
    keyfan_load(s, a.state, nv, v);
    const uint32_t cnt = min(a.in_count[p], a.in_spans);
    StageWriterT<KeyfanRows> emit{KeyfanRows{a.out, a.out.start, a.out.end, a.note_on8}, nv, v, a.max_spans, 0, 0};
    keyfan_buffer(s, a.key_freq_bits[key], key, a.out_len, cnt, a.in_start + p, a.in_end + p, a.held_lo + p, a.held_hi + p, np, emit);
    a.out.count[v] = emit.k;
    keyfan_store(s, a.state, nv, v);
    if (emit.dropped) atomicAdd(a.overflow, emit.dropped);
}
}  // namespace

struct zh_keyfan : zh_stage {
    uint32_t n_players, n_keys, nv;
    uint32_t *key_freq_bits, *state;
    uint8_t *note_on;                                                 // [rows][nv], beside the table's rows
};

namespace {
void keyfan_free(zh_keyfan *a) {
    stage_free(a->tab);
    (void)hipFree(a->note_on); (void)hipFree(a->key_freq_bits); (void)hipFree(a->state);
}
KeyfanLane keyfan_unpack(const zh_keyfan_state &h) {
    uint32_t fb;
    memcpy(&fb, &h.freq, 4);
    return KeyfanLane{h.next_id, h.down, h.has_note, h.note_id, fb, h.note_on};
}
int keyfan_upload_init(zh_keyfan *a) {                                // Voice :50-56
    if (!a->nv) return ZH_OK;
    std::vector<uint32_t> w((size_t)kKeyfanState * a->nv);
    KeyfanLane s;
    keyfan_init(s);
    for (size_t v = 0; v < a->nv; v++) keyfan_store(s, w.data(), a->nv, v);
    return zh_upload(a->ctx, a->state, w.data(), w.size() * 4);
}
}  // namespace

extern "C" {

int zh_keyfan_create(zh_ctx *ctx, uint32_t n_players, const float *key_freqs, uint32_t n_keys, zh_keyfan **out) { ZH_GUARD(ctx);
    if (!ctx || !out || !key_freqs || n_keys == 0 || n_keys > kKeyfanMaxKeys || (uint64_t)n_players * n_keys > (1ull << 31)) return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    zh_keyfan *a = new (std::nothrow) zh_keyfan();
    if (!a) return ZH_ERR_INVALID;
    memset(a, 0, sizeof *a);
    a->ctx = ctx; a->n_players = n_players; a->n_keys = n_keys; a->nv = n_players * n_keys;
    int rc = dev_alloc(&a->key_freq_bits, (size_t)n_keys);
    if (!rc) rc = dev_alloc(&a->state, (size_t)kKeyfanState * a->nv);
    if (!rc) rc = stage_create(a, a->nv, ZH_KEYFAN_SPAN_FIELDS, kKeyfanDefaultRows);
    if (!rc) rc = dev_alloc(&a->note_on, (size_t)kKeyfanDefaultRows * a->nv);
    if (!rc) rc = zh_upload(ctx, a->key_freq_bits, key_freqs, (size_t)n_keys * 4);
    if (!rc) rc = keyfan_upload_init(a);
    if (rc) return stage_create_failed(a, keyfan_free, rc);
    *out = a;
    return ZH_OK;
}

int zh_keyfan_destroy(zh_keyfan *a) { ZH_GUARD(a ? a->ctx : nullptr); return stage_destroy(a, keyfan_free); }

int zh_keyfan_reset(zh_keyfan *a) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a) return ZH_ERR_INVALID;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;                 // the upload reads host memory
    return keyfan_upload_init(a);
}

int zh_keyfan_reserve(zh_keyfan *a, uint32_t max_rows) { ZH_GUARD(a ? a->ctx : nullptr);
    const uint32_t had = a ? a->tab.rows : 0;
    int rc = stage_reserve(a, max_rows);
    if (rc || a->tab.rows == had) return rc;                          // refused, or the same capacity
    (void)hipFree(a->note_on);                                        // (the stream is idle: stage_reserve)
    rc = dev_alloc(&a->note_on, (size_t)max_rows * a->nv);
    if (rc) { stage_free_rows(a->tab); (void)hipGetLastError(); }
    return rc;
}

int zh_keyfan_schedule(zh_keyfan *a, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in, const zh_script_span_param *held) {
    ZH_GUARD(a ? a->ctx : nullptr);
    if (!stage_spans_ok(a, max_spans) || !stage_input_ok(in, false) || !held || !held[0].u || !held[1].u) return ZH_ERR_INVALID;
    if (a->nv == 0) return ZH_OK;
    const KeyfanArgs args{a->nv, a->n_players, a->n_keys, out_len, in->max_spans, max_spans, a->key_freq_bits, in->count, in->start, in->end,
                          held[0].u, held[1].u, a->state, stage_rows(a), a->note_on, a->tab.overflow};
    ZH_LAUNCH(k_keyfan_schedule, dim3((a->nv + kKeyfanBlock - 1) / kKeyfanBlock), dim3(kKeyfanBlock), 0, a->ctx->stream, args);
    return zh_launch_status();
}

int zh_keyfan_script_table(const zh_keyfan *a, uint32_t max_spans, zh_script_span_table *out) { return stage_script_table(a, max_spans, out); }
int zh_keyfan_span_param(const zh_keyfan *a, uint32_t field, zh_script_span_param *out) {
    return stage_span_param(a, field, field == ZH_KEYFAN_SPAN_FREQ ? 'f' : 'u', out);
}
int zh_keyfan_span_table(const zh_keyfan *a, uint32_t max_spans, zh_span_table *out) {
    zh_script_span_table t;
    zh_script_span_param freq;
    if (!out || stage_script_table(a, max_spans, &t) || stage_span_param(a, ZH_KEYFAN_SPAN_FREQ, 'f', &freq)) return ZH_ERR_INVALID;
    *out = zh_span_table{max_spans, 0, t.count, t.start, t.end, freq.f, a->note_on, t.note_id_changed};
    return ZH_OK;
}
int zh_keyfan_overflows(zh_keyfan *a, uint64_t *out) { ZH_GUARD(a ? a->ctx : nullptr); return stage_overflows(a, out); }

int zh_keyfan_get_state(zh_keyfan *a, zh_keyfan_state *host) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || (a->nv && !host)) return ZH_ERR_INVALID;
    if (!a->nv) return ZH_OK;
    std::vector<uint32_t> w((size_t)kKeyfanState * a->nv);
    int rc = zh_download(a->ctx, w.data(), a->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < a->nv; v++) {
        KeyfanLane s;
        keyfan_load(s, w.data(), a->nv, v);
        zh_keyfan_state h{s.next_id, s.down, s.has_note, s.note_id, 0.0f, s.note_on};
        memcpy(&h.freq, &s.freq_bits, 4);
        host[v] = h;
    }
    return ZH_OK;
}
int zh_keyfan_set_state(zh_keyfan *a, const zh_keyfan_state *host) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || (a->nv && !host)) return ZH_ERR_INVALID;
    if (!a->nv) return ZH_OK;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    std::vector<uint32_t> w((size_t)kKeyfanState * a->nv);
    for (size_t v = 0; v < a->nv; v++) keyfan_store(keyfan_unpack(host[v]), w.data(), a->nv, v);   // any words: no field indexes memory
    return zh_upload(a->ctx, a->state, w.data(), w.size() * 4);
}

}  // extern "C"
