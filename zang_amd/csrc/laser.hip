// laser.hip -- the curve-driven sound effect of examples/example_laser.zig (:22-117) as ONE fused kernel per paint:
//   k_laser<ZF>            LaserPlayer.paint for every voice, one lane per voice (:67-116)
//   k_laser_spans<ZF, TB>  MainModule's Trigger loop (:149-158) for every voice from a span table, on span_walk's segments
// and the effect kit (zh_sfx_kit) the voices play from.  Lane object, frame body, the state's and the kit's layouts: laser.hip.h;
// the handle with create / destroy / get_state / set_state: span_voice.hip.h.  The kernels stay the voice's own: the curves'
// tables live in scratch and a frame's index counts from its sub-span's start.  Not built: a wave-per-voice form for a handful of
// voices, frame ranges, a tolerant form.
#include "laser.hip.h"
#include "span_walk.hip.h"

struct zh_sfx_kit {
    zh_ctx *ctx;
    uint32_t n, array_nodes;
    zh_curve_node *nodes;                // the array of lk_pack
    LkEffectDesc *desc;
    std::vector<zh_sfx_effect> effects;  // the entries as zh_sfx_kit_effect hands them out: `nodes` point into the array
};

struct zh_laser : zh_voice {};

// the values of example_laser.zig:22-38 as {value, t}
static const zh_curve_node kLaserDefault[9] = {
    {1000.0f, 0.0f}, {200.0f, 0.1f}, {100.0f, 0.2f},        // modulator_curve :28-32
    {1000.0f, 0.0f}, {200.0f, 0.1f}, {100.0f, 0.2f},        // carrier_curve :22-26
    {0.0f, 0.0f}, {1.0f, 0.004f}, {0.0f, 0.2f},             // volume_curve :34-38
};

template <bool ZF>
__global__ void __launch_bounds__(kSeqBlock) k_laser(const LaserArgs a, const BoolP nic, const Img out, uint32_t start, uint32_t end) {
    const uint32_t v = blockIdx.x * kSeqBlock + threadIdx.x;
    if (v >= a.V) return;
    LaserLane n;
    LaserTables tb;
    n.load_state(a.state, a.V, v);
    n.begin(tb, a, a.effect.get(v), a.freq_mul.get(v), a.carrier_mul.get(v), a.modulator_mul.get(v), a.modulator_rad.get(v), end - start, nic.get(v));
    laser_paint_frames<ZF>(n, tb, out, v, start, end, start, true);
    n.end();
    n.store_state(a.state, a.V, v);
}

// TB: SpanWalkP, or OneSpanP (zh_laser_paint under the dispatch row laser_uniform_walk).  Idle lanes of the last wave shadow
// voice 0 read-only and store nothing.
template <bool ZF, class TB>
__global__ void __launch_bounds__(kSeqBlock) k_laser_spans(const LaserArgs a, const TB tb, const Img out, uint32_t start, uint32_t end) {
    const uint32_t v0 = blockIdx.x * kSeqBlock + threadIdx.x;
    const bool live = v0 < a.V;
    const uint32_t v = live ? v0 : 0;
    LaserLane n;
    LaserTables ct;
    n.load_state(a.state, a.V, v);
    const float freq_mul0 = a.freq_mul.get(v), carrier_mul0 = a.carrier_mul.get(v), modulator_mul0 = a.modulator_mul.get(v), modulator_rad0 = a.modulator_rad.get(v);
    const uint32_t effect0 = a.effect.get(v);
    uint32_t s0 = start;                                             // the running sub-span's first frame
    span_walk_segments(tb, a.V, v, live, start, end,
                       [&](size_t kv, bool nic) ZH_INLINE_LAMBDA {
                           s0 = tb.start[kv];
                           n.begin(ct, a, span_u(a.se, kv, effect0), span_f(a.sf, kv, freq_mul0), span_f(a.sc, kv, carrier_mul0), span_f(a.sm, kv, modulator_mul0),
                                   span_f(a.sr, kv, modulator_rad0), tb.end[kv] - s0, nic);
                       },
                       [&](uint32_t f0, uint32_t f1, bool active) ZH_INLINE_LAMBDA { if (live) laser_paint_frames<ZF>(n, ct, out, v, f0, f1, s0, active); },
                       [&]() ZH_INLINE_LAMBDA { n.end(); });
    if (live) n.store_state(a.state, a.V, v);
}

// what both paints check, and the kernel's arguments
static int laser_args(zh_laser *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_laser_params *p, const zh_script_span_param *sp,
                      LaserArgs &a) {
    if (!m || !outputs || !p || end < start || !buf_covers(outputs[0], m->n, end)) return ZH_ERR_INVALID;
    if (!p->kit || p->kit->ctx != m->ctx) return ZH_ERR_INVALID;
    a = LaserArgs{m->n, m->state, p->kit->nodes, p->kit->desc, p->kit->n, p->kit->array_nodes, p->sample_rate,
                  mk_f32(p->freq_mul), mk_f32(p->carrier_mul), mk_f32(p->modulator_mul), mk_f32(p->modulator_rad),
                  ZkU32P{p->effect.value, p->effect.per_voice},
                  span_fa(sp, ZH_LASER_SPAN_FREQ_MUL), span_fa(sp, ZH_LASER_SPAN_CARRIER_MUL), span_fa(sp, ZH_LASER_SPAN_MODULATOR_MUL),
                  span_fa(sp, ZH_LASER_SPAN_MODULATOR_RAD), span_ua(sp, ZH_LASER_SPAN_EFFECT)};
    return ZH_OK;
}

extern "C" {

int zh_sfx_effect_default(zh_sfx_effect *effect, zh_curve_node *nodes) {
    if (!effect || !nodes) return ZH_ERR_INVALID;
    memcpy(nodes, kLaserDefault, sizeof(kLaserDefault));
    effect->modulator = zh_sfx_curve{nodes, 3, ZH_CURVE_FN_SMOOTHSTEP};       // :79-81
    effect->carrier = zh_sfx_curve{nodes + 3, 3, ZH_CURVE_FN_SMOOTHSTEP};     // :95-97
    effect->volume = zh_sfx_curve{nodes + 6, 3, ZH_CURVE_FN_SMOOTHSTEP};      // :110-112
    return ZH_OK;
}

// lk_describe / lk_pack (laser.hip.h) lay the nodes out on the host, one copy takes the array over
int zh_sfx_kit_create(zh_ctx *ctx, const zh_sfx_effect *effects, uint32_t n, zh_sfx_kit **out) { ZH_GUARD(ctx);
    if (!ctx || !out) return ZH_ERR_INVALID;
    if (ctx->capturing) return ZH_ERR_UNSUPPORTED;                                   // the copy synchronises
    std::vector<LkEffectDesc> desc(n);
    size_t count = 0;
    int rc = lk_describe(effects, n, desc.data(), &count);
    if (rc) return rc;
    std::vector<zh_curve_node> nodes(count);
    lk_pack(effects, n, desc.data(), nodes.data(), count);
    zh_sfx_kit *k = new (std::nothrow) zh_sfx_kit();
    if (!k) return ZH_ERR_INVALID;
    k->ctx = ctx; k->n = n; k->array_nodes = (uint32_t)count; k->nodes = nullptr; k->desc = nullptr;
    k->effects.assign(effects, effects + n);
    rc = dev_alloc(&k->nodes, count);
    if (!rc) rc = dev_alloc(&k->desc, n);
    if (!rc && count) rc = zh_upload(ctx, k->nodes, nodes.data(), count * sizeof(zh_curve_node));
    if (!rc) rc = zh_upload(ctx, k->desc, desc.data(), (size_t)n * sizeof(LkEffectDesc));
    if (rc) { (void)hipFree(k->nodes); (void)hipFree(k->desc); delete k; return rc; }
    for (uint32_t i = 0; i < n; i++) {
        k->effects[i].modulator.nodes = k->nodes + desc[i].curve[LK_MODULATOR].offset;
        k->effects[i].carrier.nodes = k->nodes + desc[i].curve[LK_CARRIER].offset;
        k->effects[i].volume.nodes = k->nodes + desc[i].curve[LK_VOLUME].offset;
    }
    *out = k;
    return ZH_OK;
}
int zh_sfx_kit_destroy(zh_sfx_kit *kit) { ZH_GUARD(kit ? kit->ctx : nullptr);
    if (!kit) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(kit->ctx->stream);
    (void)hipFree(kit->nodes); (void)hipFree(kit->desc);
    delete kit;
    return ZH_OK;
}
int zh_sfx_kit_count(const zh_sfx_kit *kit, uint32_t *count_out) {
    if (!kit || !count_out) return ZH_ERR_INVALID;
    *count_out = kit->n;
    return ZH_OK;
}
int zh_sfx_kit_effect(const zh_sfx_kit *kit, uint32_t i, zh_sfx_effect *out) {
    if (!kit || !out || i >= kit->n) return ZH_ERR_INVALID;
    *out = kit->effects[i];
    return ZH_OK;
}

// init() :57-65: every word zero
int zh_laser_create(zh_ctx *ctx, uint32_t n, zh_laser **out) { ZH_GUARD(ctx); return voice_create(ctx, n, kLaserState, out); }
int zh_laser_destroy(zh_laser *m) { ZH_GUARD(m ? m->ctx : nullptr); return voice_destroy(m); }
int zh_laser_get_state(zh_laser *m, zh_laser_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_get_state<LaserLayout>(m, host); }
int zh_laser_set_state(zh_laser *m, const zh_laser_state *host) { ZH_GUARD(m ? m->ctx : nullptr); return voice_set_state<LaserLayout>(m, host); }

int zh_laser_paint(zh_laser *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, zh_bool note_id_changed,
                   const zh_laser_params *p, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    LaserArgs a;
    int rc = laser_args(m, start, end, outputs, p, nullptr, a);
    if (rc) return rc;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;         // exact forms only
    if (m->n == 0) return ZH_OK;
    const bool zf = (flags & ZH_PAINT_ZERO_FIRST) != 0;
    hipStream_t st = m->ctx->stream;
    const BoolP nic = mk_bool(note_id_changed);
    const Img out = mk_img(outputs[0]);
    if (zh_form(ZF_LASER_UNIFORM_WALK) > 0) {
        const OneSpanP tb{1, {1}, {start}, {end}, {nic}};
        if (zf) ZH_LAUNCH((k_laser_spans<true, OneSpanP>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, start, end);
        else ZH_LAUNCH((k_laser_spans<false, OneSpanP>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, tb, out, start, end);
    } else {
        if (zf) ZH_LAUNCH((k_laser<true>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, nic, out, start, end);
        else ZH_LAUNCH((k_laser<false>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, nic, out, start, end);
    }
    return zh_launch_status();
}

int zh_laser_paint_spans(zh_laser *m, uint32_t start, uint32_t end, const zh_buf *outputs, const zh_buf *temps, const zh_laser_params *p,
                         const zh_script_span_param *sp, const zh_script_span_table *table, uint32_t flags) { ZH_GUARD(m ? m->ctx : nullptr);
    (void)temps;
    static const uint8_t kinds[ZH_LASER_SPAN_FIELDS] = {SPAN_F, SPAN_F, SPAN_F, SPAN_F, SPAN_U};
    LaserArgs a;
    int rc = laser_args(m, start, end, outputs, p, sp, a);
    if (rc) return rc;
    if (!module_span_table_ok(table) || !module_span_params_ok(sp, kinds, ZH_LASER_SPAN_FIELDS)) return ZH_ERR_INVALID;
    if (flags & ZH_PAINT_TOLERANT) return ZH_ERR_UNSUPPORTED;
    if (m->n == 0) return ZH_OK;
    hipStream_t st = m->ctx->stream;
    const Img out = mk_img(outputs[0]);
    if (flags & ZH_PAINT_ZERO_FIRST) ZH_LAUNCH((k_laser_spans<true, SpanWalkP>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, mk_span_walk(table), out, start, end);
    else ZH_LAUNCH((k_laser_spans<false, SpanWalkP>), seq_grid(m->n), dim3(kSeqBlock), 0, st, a, mk_span_walk(table), out, start, end);
    return zh_launch_status();
}

}  // extern "C"
