// fm.hip -- the OPL-style two-operator FM instrument of examples/example_fmsynth.zig (:22-356) as ONE fused kernel per paint:
//   k_fm<ZF, SPLIT>        Instrument.paint for every voice, one lane per voice (:287-355)
//   k_fm_spans<ZF, SPLIT>  the synth's Trigger loop (:457-496) for every voice from a span table, on span_walk's segments
//   k_fm_patch             the 22 discrete patch values -> the numbers a paint needs (:135-203), once per set_patches
// Lane objects and the frame loop: fm.hip.h.  Not built: a wave-per-voice form for a handful of voices, frame ranges, a
// tolerant form.
#include "common.hip.h"
#include "fm.hip.h"
#include <vector>
#include <string.h>

struct zh_fm {
    zh_ctx *ctx;
    uint32_t n, group, ni;        // voices, voices per instrument, instruments = ceil(n / group)
    uint32_t *state;              // [kFmState][n]
    float *tab;                   // [kFmConsts][ni]
    uint32_t *patch;              // [ni][ZH_FM_PATCH_VALUES] staging for k_fm_patch
};

// num_values of parameters[0..21] (:376-397)
static const uint32_t kFmNumValues[ZH_FM_PATCH_VALUES] = {16, 4, 64, 16, 16, 16, 16, 2, 2, 8, 16, 4, 64, 16, 16, 16, 16, 2, 2, 2, 2, 2};
// current_value of parameters[0..21] (:376-397)
static const uint32_t kFmDefault[ZH_FM_PATCH_VALUES] = {2, 0, 0, 8, 8, 1, 8, 0, 0, 0, 1, 0, 0, 8, 8, 1, 8, 0, 0, 1, 1, 1};

__device__ __forceinline__ float fm_decibels(float db) { return zpowf(10.0f, db / 20.0f); }                 // :22-24
__device__ __forceinline__ float fm_time(uint32_t x) { return 0.002f + 4.0f * zpowf(1.0f - (float)x / 15.0f, 3.0f); }   // :160-171

// one operator's eight numbers from its discrete values (Operator.paint :135-191); `p` = the operator's first value
__device__ __forceinline__ void fm_patch_op(float *tab, uint32_t NI, uint32_t j, int op, const uint32_t *p, uint32_t trem, uint32_t vib,
                                            uint32_t trem_depth, uint32_t vib_depth) {
    float *c = tab + (size_t)op * FMC_OP * NI + j;
    const uint32_t fm = p[0], volume = p[2], sustain = p[5];
    c[(size_t)FMC_FREQ_MUL * NI] = fm == 0 ? 0.5f : fm <= 10 ? (float)fm : fm == 11 ? 10.0f : fm <= 13 ? 12.0f : 15.0f;   // :135-144
    float db = 0.0f;                                                  // 0 is the loudest, 63 the quietest (:147-156)
    if (volume & 32) db -= 24.0f;
    if (volume & 16) db -= 12.0f;
    if (volume & 8) db -= 6.0f;
    if (volume & 4) db -= 3.0f;
    if (volume & 2) db -= 1.5f;
    if (volume & 1) db -= 0.75f;
    c[(size_t)FMC_VOLUME * NI] = fm_decibels(db);
    c[(size_t)FMC_ATTACK * NI] = fm_time(p[3]);
    c[(size_t)FMC_DECAY * NI] = fm_time(p[4]);
    db = 0.0f;                                                        // :163-170
    if (sustain & 8) db -= 24.0f;
    if (sustain & 4) db -= 12.0f;
    if (sustain & 2) db -= 6.0f;
    if (sustain & 1) db -= 3.0f;
    c[(size_t)FMC_SUSTAIN * NI] = fm_decibels(db);
    c[(size_t)FMC_RELEASE * NI] = fm_time(p[6]);
    c[(size_t)FMC_TREMOLO * NI] = trem ? 1.0f - fm_decibels(trem_depth ? -4.8f : -1.0f) : 0.0f;              // :173-181
    // :183-191; the exponents are the f32 nearest 7 / 1200 and 14 / 1200
    c[(size_t)FMC_VIBRATO * NI] = vib ? zpowf(2.0f, vib_depth ? (float)(14.0 / 1200.0) : (float)(7.0 / 1200.0)) - 1.0f : 0.0f;
}

// patches: [n_patches][22]; n_patches == 1: the one patch for every instrument
__global__ void __launch_bounds__(64) k_fm_patch(float *tab, uint32_t NI, const uint32_t *patches, uint32_t n_patches) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= NI) return;
    const uint32_t *p = patches + (size_t)(n_patches == 1 ? 0 : j) * ZH_FM_PATCH_VALUES;
    const uint32_t td = p[ZH_FM_TREMOLO_DEPTH], vd = p[ZH_FM_VIBRATO_DEPTH];
    fm_patch_op(tab, NI, j, 0, p + ZH_FM_MOD_FREQ_MUL, p[ZH_FM_MOD_TREMOLO], p[ZH_FM_MOD_VIBRATO], td, vd);
    fm_patch_op(tab, NI, j, 1, p + ZH_FM_CAR_FREQ_MUL, p[ZH_FM_CAR_TREMOLO], p[ZH_FM_CAR_VIBRATO], td, vd);
    const float pi = 3.14159265358979323846f;                         // :193-203
    const uint32_t fb = p[ZH_FM_MOD_FEEDBACK];
    tab[(size_t)FMC_FEEDBACK * NI + j] = fb == 0 ? 0.0f : fb == 1 ? pi / 16.0f : fb == 2 ? pi / 8.0f : fb == 3 ? pi / 4.0f : fb == 4 ? pi / 2.0f :
                                         fb == 5 ? pi : fb == 6 ? pi * 2.0f : pi * 4.0f;
    tab[(size_t)FMC_BITS * NI + j] = zbits_f((p[ZH_FM_ALGORITHM] & 1u) | (p[ZH_FM_MOD_WAVEFORM] & 3u) << 1 | (p[ZH_FM_CAR_WAVEFORM] & 3u) << 3);
}

// does any lane of the wave have waveform 3 on either operator?  (wave-uniform; idle lanes shadow a live voice's patch)
__device__ __forceinline__ bool fm_any3(const FMLane &n) { return zany_wave(n.mod.waveform == 3 || n.car.waveform == 3); }

template <bool ZF, bool SPLIT>
__global__ void __launch_bounds__(kSeqBlock) k_fm(FMArgs a, Img out, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;                                 // idle lanes shadow voice 0 read-only and store nothing
    const uint32_t j = v / a.group;
    FMLane n;
    n.load_consts(a.tab, a.NI, j);
    n.load_state(a.state, a.V, v);
    const bool any3 = fm_any3(n);
    if (!live) return;
    n.begin(a.sample_rate, a.freq.get(v), a.note_on.get(v), a.nic.get(v));
    fm_paint_frames<ZF, SPLIT>(n, out, v, a, j, start, end, true, any3);
    n.end();
    n.store_state(a.state, a.V, v);
}

template <bool ZF, bool SPLIT>
__global__ void __launch_bounds__(kSeqBlock) k_fm_spans(FMArgs a, NoteSpanTableP tb, Img out, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    const uint32_t j = v / a.group;
    FMLane n;
    n.load_consts(a.tab, a.NI, j);
    n.load_state(a.state, a.V, v);
    const bool any3 = fm_any3(n);
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA { n.begin(a.sample_rate, tb.freq[kv], tb.note_on[kv] != 0, nic); },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA { if (live) fm_paint_frames<ZF, SPLIT>(n, out, v, a, j, f0, f1, active, any3); },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}

static void fm_free(zh_fm *m) { (void)hipFree(m->state); (void)hipFree(m->tab); (void)hipFree(m->patch); }

// validate, stage and convert; nothing changes unless every value is inside its num_values
static int fm_set_patches(zh_fm *m, const zh_fm_patch *patches, uint32_t n_patches) {
    if (!patches || (n_patches != 1 && n_patches != m->ni)) return ZH_ERR_INVALID;
    for (uint32_t i = 0; i < n_patches; i++)
        for (int k = 0; k < ZH_FM_PATCH_VALUES; k++)
            if (patches[i].value[k] >= kFmNumValues[k]) return ZH_ERR_INVALID;      // the reference's `unreachable` arms
    if (m->ctx->capturing) return ZH_ERR_UNSUPPORTED;                 // (a host copy and a synchronisation)
    if (m->ni == 0) return ZH_OK;
    int rc = zh_upload(m->ctx, m->patch, patches, (size_t)n_patches * sizeof(zh_fm_patch));
    if (rc) return rc;
    ZH_LAUNCH(k_fm_patch, dim3((m->ni + 63) / 64), dim3(64), 0, m->ctx->stream, m->tab, m->ni, m->patch, n_patches);
    return zh_launch_status();
}

extern "C" {

int zh_fm_patch_default(zh_fm_patch *patch) {
    if (!patch) return ZH_ERR_INVALID;
    memcpy(patch->value, kFmDefault, sizeof(kFmDefault));
    return ZH_OK;
}

int zh_fm_create(zh_ctx *ctx, uint32_t n, uint32_t group, zh_fm **out) { ZH_GUARD(ctx);
    if (!ctx || !out || group == 0) return ZH_ERR_INVALID;
    zh_fm *m = new (std::nothrow) zh_fm();
    if (!m) return ZH_ERR_INVALID;
    m->ctx = ctx; m->n = n; m->group = group; m->ni = (uint32_t)(((uint64_t)n + group - 1) / group);
    m->state = nullptr; m->tab = nullptr; m->patch = nullptr;
    int rc = dev_alloc_zeroed(ctx, &m->state, (size_t)kFmState * n);
    if (!rc) rc = dev_alloc(&m->tab, (size_t)kFmConsts * m->ni);
    if (!rc) rc = dev_alloc(&m->patch, (size_t)ZH_FM_PATCH_VALUES * m->ni);
    if (!rc) {
        zh_fm_patch d;
        memcpy(d.value, kFmDefault, sizeof(kFmDefault));
        rc = fm_set_patches(m, &d, 1);
    }
    if (rc) { fm_free(m); delete m; return rc; }
    *out = m;
    return ZH_OK;
}

int zh_fm_destroy(zh_fm *m) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    fm_free(m);
    delete m;
    return ZH_OK;
}

int zh_fm_set_patches(zh_fm *m, const zh_fm_patch *patches, uint32_t n_patches) { ZH_GUARD(m ? m->ctx : nullptr);
    if (!m) return ZH_ERR_INVALID;
    return fm_set_patches(m, patches, n_patches);
}

int zh_fm_get_state(zh_fm *m, zh_fm_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    return m && host ? block_get_state<FmLayout>(m->ctx, m->state, m->n, host) : ZH_ERR_INVALID;
}
int zh_fm_set_state(zh_fm *m, const zh_fm_state *host) { ZH_GUARD(m ? m->ctx : nullptr);
    return m && host ? block_set_state<FmLayout>(m->ctx, m->state, m->n, host) : ZH_ERR_INVALID;
}

// the checks both paints share; on ZH_OK `flags` has lost ZH_PAINT_ZERO_FIRST where an LFO image overlaps the output (zeroed here)
static int fm_paint_check(zh_fm *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf &trem, const zh_buf &vib, uint32_t &flags) {
    if (end < start) return ZH_ERR_INVALID;
    const uint64_t cols = (flags & ZH_FM_SPLIT_OPERATORS) ? 2ull * m->n : m->n;
    if (cols > 0xffffffffull || !buf_covers(outputs[0], (uint32_t)cols, end)) return ZH_ERR_INVALID;
    if (!buf_covers(trem, m->ni, end) || !buf_covers(vib, m->ni, end)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    return zh_zero_first_aliased(m->ctx, start, end, outputs[0], (uint32_t)cols, bufs_alias(trem, outputs[0]) || bufs_alias(vib, outputs[0]), flags);
}

#define ZH_FM_LAUNCH(NAME, ...)                                                                                                   \
    do {                                                                                                                          \
        const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0, split = (flags & ZH_FM_SPLIT_OPERATORS) != 0;                         \
        if (zf) { if (split) ZH_LAUNCH((NAME<true, true>), seq_grid(m->n), dim3(kSeqBlock), 0, st, __VA_ARGS__);                  \
                  else ZH_LAUNCH((NAME<true, false>), seq_grid(m->n), dim3(kSeqBlock), 0, st, __VA_ARGS__); }                     \
        else { if (split) ZH_LAUNCH((NAME<false, true>), seq_grid(m->n), dim3(kSeqBlock), 0, st, __VA_ARGS__);                    \
               else ZH_LAUNCH((NAME<false, false>), seq_grid(m->n), dim3(kSeqBlock), 0, st, __VA_ARGS__); }                       \
    } while (0)

int zh_fm_paint(zh_fm *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                const zh_fm_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    if (!m || !outputs || !p) return ZH_ERR_INVALID;
    int rc = fm_paint_check(m, start, end, outputs, p->tremolo_input, p->vibrato_input, flags);
    if (rc) return rc;
    if (m->n == 0) return ZH_OK;
    hipStream_t st = m->ctx->stream;
    FMArgs a{m->state, m->tab, m->n, m->ni, m->group, p->sample_rate, mk_cimg(p->tremolo_input), mk_cimg(p->vibrato_input),
             mk_f32(p->freq), mk_bool(p->note_on), mk_bool(note_id_changed)};
    ZH_FM_LAUNCH(k_fm, a, mk_img(outputs[0]), start, end);
    return zh_launch_status();
}

int zh_fm_paint_spans(zh_fm *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, float sample_rate,
                      zh_buf tremolo_input, zh_buf vibrato_input, const zh_span_table *t, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    if (!m || !outputs) return ZH_ERR_INVALID;
    if (!note_span_table_ok(t)) return ZH_ERR_INVALID;
    int rc = fm_paint_check(m, start, end, outputs, tremolo_input, vibrato_input, flags);
    if (rc) return rc;
    if (m->n == 0) return ZH_OK;
    hipStream_t st = m->ctx->stream;
    FMArgs a{m->state, m->tab, m->n, m->ni, m->group, sample_rate, mk_cimg(tremolo_input), mk_cimg(vibrato_input),
             F32P{0.0f, nullptr}, BoolP{0, nullptr}, BoolP{0, nullptr}};
    ZH_FM_LAUNCH(k_fm_spans, a, mk_note_span_table(t), mk_img(outputs[0]), start, end);
    return zh_launch_status();
}

}  // extern "C"
