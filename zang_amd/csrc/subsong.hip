// subsong.hip -- the subsong stage: SubtrackPlayer.paint of examples/example_subsong.zig (:122-144) without its instrument, for n
// players on the device, and the melodies it plays as a device-resident kit (zh_melody_kit_*: K songs of notes.zig:130-134 in one
// blob, CSR-shaped).  k_subsong_schedule, one lane per player, reads the sub-span table a live voice bank of polyphony 1 filled from
// the records {freq, note_on, melody} (MainModule.paint :176-185) and writes the stage's own [span][player] table, which the span
// paints read in place.  The per-lane steps are subsong_lane.hip.h; semantics and what is defined where the reference is not:
// zang_hip.h.
#include "common.hip.h"
#include "subsong_lane.hip.h"
#include "span_stage.hip.h"
#include <vector>
#include <string.h>

namespace {
constexpr uint32_t kSubsongBlock = 64;
constexpr uint32_t kSubsongDefaultRows = 33;                          // what one outer sub-span can make: the carried note + 32 impulses
static_assert(kSubsongNoMelody == UINT32_MAX, "the value zang_hip.h documents");
static_assert(ZH_SUBSONG_SPAN_FREQ == 0 && ZH_SUBSONG_SPAN_NOTE_ON == 1 && ZH_SUBSONG_SPAN_FIELDS == 2, "the fields StageWriter emits");

struct SubsongArgs {
    uint32_t n, out_len, in_spans, max_spans;
    float sample_rate, base_freq;
    SubsongKitP kit;
    const uint32_t *in_count, *in_start, *in_end;                     // the outer table, [in_spans][n]
    const uint8_t *in_nic;
    const float *in_freq;
    const uint32_t *in_note_on, *in_melody;
    uint32_t *state;                                                  // [kSubsongState][n]
    StageRows out;                                                    // the stage's table: fields ZH_SUBSONG_SPAN_FREQ, _NOTE_ON
    uint32_t *overflow;
};

__global__ void __launch_bounds__(kSubsongBlock) k_subsong_schedule(const SubsongArgs a) {
    const uint32_t p = blockIdx.x * kSubsongBlock + threadIdx.x;
    if (p >= a.n) return;
    const size_t n = a.n;
    SubsongLane s;
    subsong_load(s, a.state, n, p);
    const uint32_t cnt = min(a.in_count[p], a.in_spans);
    StageWriter emit{a.out, n, p, a.max_spans, 0, 0};
    subsong_buffer(s, a.kit, a.base_freq, a.sample_rate, a.out_len, cnt, a.in_start + p, a.in_end + p, a.in_nic + p, a.in_freq + p,
                   a.in_note_on + p, a.in_melody + p, n, emit);
    a.out.count[p] = emit.k;
    subsong_store(s, a.state, n, p);
    if (emit.dropped) atomicAdd(a.overflow, emit.dropped);
}
}  // namespace

struct zh_melody_kit {
    zh_ctx *ctx;
    uint32_t K, events;
    uint32_t *blob;                                                   // offsets[K + 1], then five rows of `events` words
    SubsongKitP p;
};

struct zh_subsong : zh_stage {
    const zh_melody_kit *kit;
    uint32_t n;
    float base_freq;
    uint32_t *state;
};

namespace {
void subsong_free(zh_subsong *a) {
    stage_free(a->tab);
    (void)hipFree(a->state);
}
int subsong_upload_init(zh_subsong *a) {                              // init() :104-120
    if (!a->n) return ZH_OK;
    std::vector<uint32_t> w((size_t)kSubsongState * a->n);
    SubsongLane s;
    subsong_init(s, a->kit->K);
    for (size_t v = 0; v < a->n; v++) subsong_store(s, w.data(), a->n, v);
    return zh_upload(a->ctx, a->state, w.data(), w.size() * 4);
}
}  // namespace

extern "C" {

int zh_melody_kit_create(zh_ctx *ctx, const uint32_t *offsets, uint32_t n_melodies, const zh_melody_event *events, uint32_t n_events,
                         zh_melody_kit **out) { ZH_GUARD(ctx);
    if (!ctx || !out || !offsets || (n_events && !events) || n_melodies == 0xffffffffu) return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    for (uint32_t m = 0; m <= n_melodies; m++) {
        if (offsets[m] > n_events) return ZH_ERR_INVALID;             // runs past the events
        if (m && offsets[m] < offsets[m - 1]) return ZH_ERR_INVALID;
    }
    for (uint32_t m = 0; m < n_melodies; m++)                         // a song is chronological (notes.zig:177)
        for (uint32_t e = offsets[m]; e < offsets[m + 1]; e++) {
            const float t = events[e].t;
            if (!(t >= 0.0f)) return ZH_ERR_INVALID;                  // NaN too
            if (e > offsets[m] && t < events[e - 1].t) return ZH_ERR_INVALID;
        }
    zh_melody_kit *k = new (std::nothrow) zh_melody_kit();
    if (!k) return ZH_ERR_INVALID;
    memset(k, 0, sizeof *k);
    k->ctx = ctx; k->K = n_melodies; k->events = n_events;
    const size_t no = (size_t)n_melodies + 1, ne = n_events;
    std::vector<uint32_t> w(no + 5 * ne);
    for (size_t m = 0; m < no; m++) w[m] = offsets[m];
    for (size_t e = 0; e < ne; e++) {
        memcpy(&w[no + e], &events[e].t, 4);
        w[no + ne + e] = (uint32_t)events[e].note_id; w[no + 2 * ne + e] = (uint32_t)(events[e].note_id >> 32);
        memcpy(&w[no + 3 * ne + e], &events[e].freq, 4);
        w[no + 4 * ne + e] = events[e].note_on ? 1u : 0u;
    }
    int rc = dev_alloc(&k->blob, w.size());
    if (!rc) rc = zh_upload(ctx, k->blob, w.data(), w.size() * 4);
    if (rc) { (void)hipFree(k->blob); delete k; (void)hipGetLastError(); return rc; }
    const uint32_t *b = k->blob;
    k->p = SubsongKitP{n_melodies, b, b + no, b + no + ne, b + no + 2 * ne, b + no + 3 * ne, b + no + 4 * ne};
    *out = k;
    return ZH_OK;
}
int zh_melody_kit_destroy(zh_melody_kit *kit) { ZH_GUARD(kit ? kit->ctx : nullptr);
    if (!kit) return ZH_ERR_INVALID;
    if (!kit->ctx->capturing) (void)hipStreamSynchronize(kit->ctx->stream);
    (void)hipFree(kit->blob);
    delete kit;
    return ZH_OK;
}
int zh_melody_kit_count(const zh_melody_kit *kit, uint32_t *melodies_out, uint32_t *events_out) {
    if (!kit || !melodies_out) return ZH_ERR_INVALID;
    *melodies_out = kit->K;
    if (events_out) *events_out = kit->events;
    return ZH_OK;
}

int zh_subsong_create(zh_ctx *ctx, uint32_t n_players, const zh_melody_kit *kit, float base_freq, zh_subsong **out) { ZH_GUARD(ctx);
    if (!ctx || !out || !kit || kit->ctx != ctx || base_freq != base_freq || n_players > (1u << 31)) return ZH_ERR_INVALID;
    *out = nullptr;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;
    zh_subsong *a = new (std::nothrow) zh_subsong();
    if (!a) return ZH_ERR_INVALID;
    memset(a, 0, sizeof *a);
    a->ctx = ctx; a->kit = kit; a->n = n_players; a->base_freq = base_freq;
    int rc = dev_alloc(&a->state, (size_t)kSubsongState * n_players);
    if (!rc) rc = stage_create(a, n_players, ZH_SUBSONG_SPAN_FIELDS, kSubsongDefaultRows);
    if (!rc) rc = subsong_upload_init(a);
    if (rc) return stage_create_failed(a, subsong_free, rc);
    *out = a;
    return ZH_OK;
}

int zh_subsong_destroy(zh_subsong *a) { ZH_GUARD(a ? a->ctx : nullptr); return stage_destroy(a, subsong_free); }

int zh_subsong_reset(zh_subsong *a) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a) return ZH_ERR_INVALID;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;                 // the upload reads host memory
    return subsong_upload_init(a);
}

int zh_subsong_reserve(zh_subsong *a, uint32_t max_rows) { ZH_GUARD(a ? a->ctx : nullptr); return stage_reserve(a, max_rows); }

int zh_subsong_schedule(zh_subsong *a, float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in,
                        const zh_script_span_param *outer) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!stage_spans_ok(a, max_spans) || !stage_input_ok(in, true) || !outer || !outer[ZH_SUBSONG_IN_FREQ].f ||
        !outer[ZH_SUBSONG_IN_NOTE_ON].u || !outer[ZH_SUBSONG_IN_MELODY].u)
        return ZH_ERR_INVALID;
    if (a->n == 0) return ZH_OK;
    const SubsongArgs args{a->n, out_len, in->max_spans, max_spans, sample_rate, a->base_freq, a->kit->p, in->count, in->start, in->end,
                           in->note_id_changed, outer[ZH_SUBSONG_IN_FREQ].f, outer[ZH_SUBSONG_IN_NOTE_ON].u, outer[ZH_SUBSONG_IN_MELODY].u,
                           a->state, stage_rows(a), a->tab.overflow};
    ZH_LAUNCH(k_subsong_schedule, dim3((a->n + kSubsongBlock - 1) / kSubsongBlock), dim3(kSubsongBlock), 0, a->ctx->stream, args);
    return zh_launch_status();
}

int zh_subsong_script_table(const zh_subsong *a, uint32_t max_spans, zh_script_span_table *out) { return stage_script_table(a, max_spans, out); }
int zh_subsong_span_param(const zh_subsong *a, uint32_t field, zh_script_span_param *out) {
    return stage_span_param(a, field, field == ZH_SUBSONG_SPAN_FREQ ? 'f' : 'u', out);
}
int zh_subsong_overflows(zh_subsong *a, uint64_t *out) { ZH_GUARD(a ? a->ctx : nullptr); return stage_overflows(a, out); }

int zh_subsong_get_state(zh_subsong *a, zh_subsong_state *host) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || (a->n && !host)) return ZH_ERR_INVALID;
    if (!a->n) return ZH_OK;
    std::vector<uint32_t> w((size_t)kSubsongState * a->n);
    int rc = zh_download(a->ctx, w.data(), a->state, w.size() * 4);
    if (rc) return rc;
    for (size_t v = 0; v < a->n; v++) {
        SubsongLane s;
        subsong_load(s, w.data(), a->n, v);
        zh_subsong_state h{s.next, 0.0f, s.melody, s.has_note, s.note_id, 0.0f, s.note_on};
        memcpy(&h.t, &s.t_bits, 4);
        memcpy(&h.freq, &s.freq_bits, 4);
        host[v] = h;
    }
    return ZH_OK;
}
int zh_subsong_set_state(zh_subsong *a, const zh_subsong_state *host) { ZH_GUARD(a ? a->ctx : nullptr);
    if (!a || (a->n && !host)) return ZH_ERR_INVALID;
    if (!a->n) return ZH_OK;
    if (a->ctx->capturing) return ZH_ERR_UNSUPPORTED;
    std::vector<uint32_t> w((size_t)kSubsongState * a->n);
    for (size_t v = 0; v < a->n; v++) {
        const zh_subsong_state &h = host[v];
        if (h.melody >= a->kit->K && h.melody != kSubsongNoMelody) return ZH_ERR_INVALID;   // it indexes the kit
        uint32_t tb, fb;
        memcpy(&tb, &h.t, 4);
        memcpy(&fb, &h.freq, 4);
        subsong_store(SubsongLane{h.next_song_event, tb, h.melody, h.has_note, h.note_id, fb, h.note_on}, w.data(), a->n, v);
    }
    return zh_upload(a->ctx, a->state, w.data(), w.size() * 4);
}

}  // extern "C"
