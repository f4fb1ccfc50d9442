// harness.cpp -- random sequences through the C ABI against libzang_hip built host-only with ASan + UBSan over hip_stub.cpp
// (tools/host_asan.sh): begin_capture (with and without ZH_CAPTURE_COALESCE), paints of flipper modules (PulseOsc / TriSawOsc in
// table form, SineOsc as frame ranges; Envelope, Decimator and PMOsc: blocks of 4, 2 and 6 words per voice through the shared
// create / destroy / get_state / set_state of csrc/state_block.hip.h), held-back batches (oscillators, stereo mixdowns), the pipelined Noise -> Filter recording,
// eager paints between replays, end / launch / destroy in every order -- modules before their graphs, the context before its graphs.
// Before them, once with no player and once with five: a live bank and each span-table stage (arp, subsong, merge) through create,
// reserve, views, schedule, overflows and destroy (stage_passes).
// No kernel runs: what is checked is the host bookkeeping (ctx.hip, osc.hip, composite.hip, basics.hip) for memory errors, and at
// the end that no device allocation, stream or graph is left.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zang_hip.h"
extern "C" void hip_stub_report(unsigned long *, unsigned long *, unsigned long *, unsigned long *, unsigned long *);

static unsigned long long rs = 88172645463325252ull;
static unsigned rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (unsigned)(rs >> 11); }
static unsigned pick(unsigned n) { return rnd() % n; }
#define OK(x) do { int rc_ = (x); if (rc_ != ZH_OK) { fprintf(stderr, "%s:%d: %s -> %d\n", __FILE__, __LINE__, #x, rc_); exit(1); } } while (0)

enum Kind { PULSE, TRISAW, SINE, NF, NICE, ENV, DECIM, PMOSC, NKIND };
struct Mod { Kind kind; void *h; unsigned V; float *freq, *color; bool painted; };
struct Ctx {
    zh_ctx *c;
    std::vector<Mod> mods;
    std::vector<zh_graph *> graphs;
    std::vector<zh_buf> imgs;            // [1024][V] images by voice count (made on demand)
    float *mix;                          // 64 rows of 1,024 floats
    bool capturing; unsigned flags;
};
static const unsigned kVoices[] = {64, 300, 4096, 20000};
static zh_f32 f32c(float v) { zh_f32 x; memset(&x, 0, sizeof x); x.value = v; return x; }
static zh_f32 f32p(const float *p) { zh_f32 x; memset(&x, 0, sizeof x); x.per_voice = p; return x; }
static zh_bool boolc(unsigned v) { zh_bool x; memset(&x, 0, sizeof x); x.value = v; return x; }
static zh_cob cobc(zh_f32 c) { zh_cob x; memset(&x, 0, sizeof x); x.tag = ZH_COB_CONSTANT; x.constant = c; return x; }

static zh_buf image(Ctx &cx, unsigned V, unsigned which) {
    for (unsigned tries = 0;; tries++) {
        unsigned n = 0;
        for (zh_buf &b : cx.imgs) if (b.voices == V && n++ == which) return b;
        zh_buf b;
        OK(zh_buf_alloc(cx.c, &b, V, 1024));
        cx.imgs.push_back(b);
    }
}
static void add_module(Ctx &cx) {
    Mod m; m.kind = (Kind)pick(NKIND); m.V = kVoices[pick(4)]; m.h = nullptr; m.painted = false;
    OK(zh_malloc(cx.c, (void **)&m.freq, (size_t)m.V * 4)); OK(zh_malloc(cx.c, (void **)&m.color, (size_t)m.V * 4));
    switch (m.kind) {
    case PULSE: OK(zh_pulseosc_create(cx.c, m.V, (zh_pulseosc **)&m.h)); break;
    case TRISAW: OK(zh_trisawosc_create(cx.c, m.V, (zh_trisawosc **)&m.h)); break;
    case SINE: OK(zh_sineosc_create(cx.c, m.V, (zh_sineosc **)&m.h)); break;
    case NF: OK(zh_noise_filter_create(cx.c, m.V, 7, (zh_noise_filter **)&m.h)); break;
    case ENV: OK(zh_envelope_create(cx.c, m.V, (zh_envelope **)&m.h)); break;
    case DECIM: OK(zh_decimator_create(cx.c, m.V, (zh_decimator **)&m.h)); break;
    case PMOSC: OK(zh_pmosc_create(cx.c, m.V, f32p(m.color), (zh_pmosc **)&m.h)); break;
    default: OK(zh_nice_create(cx.c, m.V, f32p(m.color), (zh_nice **)&m.h)); break;
    }
    cx.mods.push_back(m);
}
static void drop_module(Ctx &cx, size_t i) {
    Mod &m = cx.mods[i];
    switch (m.kind) {
    case PULSE: OK(zh_pulseosc_destroy((zh_pulseosc *)m.h)); break;
    case TRISAW: OK(zh_trisawosc_destroy((zh_trisawosc *)m.h)); break;
    case SINE: OK(zh_sineosc_destroy((zh_sineosc *)m.h)); break;
    case NF: OK(zh_noise_filter_destroy((zh_noise_filter *)m.h)); break;
    case ENV: OK(zh_envelope_destroy((zh_envelope *)m.h)); break;
    case DECIM: OK(zh_decimator_destroy((zh_decimator *)m.h)); break;
    case PMOSC: OK(zh_pmosc_destroy((zh_pmosc *)m.h)); break;
    default: OK(zh_nice_destroy((zh_nice *)m.h)); break;
    }
    OK(zh_free(cx.c, m.freq)); OK(zh_free(cx.c, m.color));
    cx.mods.erase(cx.mods.begin() + (long)i);
}
// one paint; inside a capture the return code may be ZH_ERR_UNSUPPORTED (a scratch that cannot grow while recording): allowed
struct Fixed { bool on; unsigned s, e, zf, tol, nic; };
static void paint(Ctx &cx, Mod &m, const Fixed *fx = nullptr) {
    const bool whole = pick(3) != 0;
    unsigned s = whole ? 0 : pick(900), e = whole ? 1024 : s + pick(1024 - s) + 1;
    unsigned flags = (pick(2) ? ZH_PAINT_ZERO_FIRST : 0);
    if (fx) { s = fx->s; e = fx->e; flags = fx->zf ? ZH_PAINT_ZERO_FIRST : 0; }
    static unsigned next_img = 0;
    zh_buf out = image(cx, m.V, cx.capturing ? (pick(5) ? next_img++ % 12 : pick(12)) : pick(3));   // mostly a ring of images (batches form), now and then one again
    int rc = ZH_OK;
    switch (m.kind) {
    case PULSE: case TRISAW: {
        if (m.painted && (fx || pick(4))) flags |= ZH_PAINT_PARAMS_UNCHANGED;
        if (m.kind == PULSE) { zh_pulseosc_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.freq = cobc(f32p(m.freq)); p.color = f32p(m.color);
            rc = zh_pulseosc_paint((zh_pulseosc *)m.h, s, e, &out, nullptr, boolc(0), &p, flags); }
        else { zh_trisawosc_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.freq = cobc(f32p(m.freq)); p.color = f32p(m.color);
            rc = zh_trisawosc_paint((zh_trisawosc *)m.h, s, e, &out, nullptr, boolc(0), &p, flags); }
        break; }
    case SINE: { zh_sineosc_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.freq = cobc(f32p(m.freq)); p.phase = cobc(f32c(0.25f));
        if (pick(2)) flags |= ZH_PAINT_TOLERANT;
        rc = zh_sineosc_paint((zh_sineosc *)m.h, s, e, &out, nullptr, boolc(0), &p, flags); break; }
    case NF: { zh_noise_filter_params p; memset(&p, 0, sizeof p); p.color = ZH_NOISE_WHITE; p.type = 1 + pick(5); p.cutoff = f32p(m.freq); p.res = f32c(0.5f);
        if (fx ? fx->tol : pick(3)) flags |= ZH_PAINT_TOLERANT;
        rc = zh_noise_filter_paint((zh_noise_filter *)m.h, s, e, &out, nullptr, boolc(0), &p, flags); break; }
    case ENV: { zh_envelope_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.attack.tag = p.decay.tag = p.release.tag = ZH_CURVE_CUBED;
        p.attack.duration = f32c(0.004f); p.decay.duration = f32p(m.color); p.release.duration = f32c(0.03f); p.sustain_volume = f32c(0.6f); p.note_on = boolc(pick(2));
        rc = zh_envelope_paint((zh_envelope *)m.h, s, e, &out, nullptr, boolc(pick(2)), &p, flags); break; }
    case DECIM: { zh_decimator_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.input = image(cx, m.V, 12); p.fake_sample_rate = f32p(m.freq);   // (image 12: never an output)
        if (!fx && !pick(4)) {   // an in-place span paint: the input IS the output, so ZERO_FIRST zeroes the span before the paint (any device address passes as a table array)
            const zh_script_span_table t{1, 0, (const uint32_t *)m.freq, (const uint32_t *)m.color, (const uint32_t *)m.color, (const uint8_t *)m.freq};
            p.input = out;
            rc = zh_decimator_paint_spans((zh_decimator *)m.h, s, e, &out, nullptr, &p, nullptr, &t, ZH_PAINT_ZERO_FIRST); break; }
        rc = zh_decimator_paint((zh_decimator *)m.h, s, e, &out, nullptr, boolc(0), &p, flags); break; }
    case PMOSC: { zh_pmosc_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.freq = f32p(m.freq); p.note_on = boolc(pick(2));
        rc = zh_pmosc_paint((zh_pmosc *)m.h, s, e, &out, nullptr, boolc(pick(2)), &p, flags); break; }
    default: { zh_nice_params p; memset(&p, 0, sizeof p); p.sample_rate = 48000.0f; p.freq = f32p(m.freq); p.note_on = boolc(pick(2));
        static unsigned next_row = 0;
        const unsigned row = fx ? next_row++ % 31 : pick(31);
        rc = zh_nice_paint_mix_stereo((zh_nice *)m.h, s, e, cx.mix + (size_t)row * 2048, cx.mix + (size_t)row * 2048 + 1024, f32p(m.color), (fx ? fx->nic : pick(2)) ? f32p(m.freq) : f32p(m.color),
                                      boolc(pick(2)), &p, flags | ((fx ? fx->tol : !pick(4)) ? ZH_PAINT_TOLERANT : 0u)); break; }
    }
    if (rc != ZH_OK && !(cx.capturing && rc == ZH_ERR_UNSUPPORTED)) { fprintf(stderr, "paint kind %d V %u span (%u, %u) flags %u -> %d\n", (int)m.kind, m.V, s, e, flags, rc); exit(1); }
    m.painted = rc == ZH_OK;
}

// The table of one stage, or of a bank, through what they share (csrc/span_stage.hip.h): reserve up, down and to the same
// capacity, the refusals at the capacity's edges, every view, the overflow count.  Leaves a capacity of `rows`.
#define MUST(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #x); exit(1); } } while (0)
template <class H>
static void table_pass(H *h, int (*reserve)(H *, uint32_t), int (*table)(const H *, uint32_t, zh_script_span_table *),
                       int (*param)(const H *, uint32_t, zh_script_span_param *), int (*overflows)(H *, uint64_t *), unsigned fields, unsigned rows, unsigned n) {
    zh_script_span_table t, same;
    zh_script_span_param p, next;
    OK(reserve(h, 64)); OK(reserve(h, 2)); OK(reserve(h, rows));
    OK(table(h, rows, &t));
    OK(reserve(h, rows));                                             // the same capacity: the views stay
    OK(table(h, rows, &same));
    MUST(same.count == t.count && same.start == t.start && same.end == t.end && same.note_id_changed == t.note_id_changed);
    MUST((t.start != nullptr) == (n != 0));
    MUST(reserve(h, 0) == ZH_ERR_INVALID && table(h, 0, &same) == ZH_ERR_INVALID && table(h, rows + 1, &same) == ZH_ERR_INVALID);
    for (unsigned f = 0; f < fields; f++) {
        OK(param(h, f, &p));
        MUST(!n || p.f || p.u);
        if (n && f + 1 < fields) {                                    // one block: fields a plane of capacity x n words apart
            OK(param(h, f + 1, &next));
            const uint32_t *a = p.u ? p.u : (const uint32_t *)p.f, *b = next.u ? next.u : (const uint32_t *)next.f;
            MUST(b - a == (ptrdiff_t)rows * n);
        }
    }
    MUST(param(h, fields, &p) == ZH_ERR_INVALID);
    uint64_t dropped = 1;
    OK(overflows(h, &dropped));
    MUST(dropped == 0);
}
// one pass per stage over a live bank of polyphony 1, n players: create, table_pass, schedule, overflows, destroy
static void stage_passes(unsigned n) {
    zh_ctx *c;
    OK(zh_create(&c, 0));
    const unsigned kRows = 7, kWords = 3;
    uint64_t dropped = 1;
    zh_voice_bank *bank;
    OK(zh_voice_bank_create_live(c, n, 1, kWords * 4, 8, 16, &bank));
    table_pass(bank, zh_voice_bank_reserve, zh_voice_bank_script_table, zh_voice_bank_span_param, zh_voice_bank_overflows, kWords, kRows, n);
    zh_span_table st;
    OK(zh_voice_bank_span_table(bank, kRows, 0, &st));
    MUST(zh_voice_bank_span_table(bank, kRows + 1, 0, &st) == ZH_ERR_INVALID && zh_voice_bank_span_table(bank, kRows, kWords, &st) == ZH_ERR_INVALID);
    std::vector<uint32_t> inst, frame, rec;
    std::vector<uint64_t> ids;
    for (unsigned i = 0; i < n; i++) { inst.push_back(n - 1 - i); frame.push_back(i); ids.push_back(i + 1); rec.insert(rec.end(), {i, 0u, 1u}); }
    const zh_bank_impulses batch{n, inst.data(), frame.data(), ids.data(), rec.data()};
    MUST(zh_voice_bank_schedule_live(bank, 64, kRows + 1, &batch) == ZH_ERR_INVALID);
    OK(zh_voice_bank_schedule_live(bank, 64, kRows, n ? &batch : nullptr));
    OK(zh_voice_bank_overflows(bank, &dropped));
    MUST(dropped == 0);
    zh_script_span_table in;
    zh_script_span_param w[kWords], f0 = {}, u1 = {}, u2 = {};
    OK(zh_voice_bank_script_table(bank, kRows, &in));
    for (unsigned k = 0; k < kWords; k++) OK(zh_voice_bank_span_param(bank, k, &w[k]));
    f0.f = w[0].f; u1.u = w[1].u; u2.u = w[2].u;
    if (!n) { static const uint32_t none = 0; in.count = in.start = in.end = &none; in.note_id_changed = (const uint8_t *)&none; f0.f = (const float *)&none; u1.u = u2.u = &none; }   // no player, no arrays: any address passes the checks

    const float keys[3] = {220.0f, 330.0f, 440.0f};
    zh_arp *arp;
    OK(zh_arp_create(c, n, keys, 3, &arp));
    table_pass(arp, zh_arp_reserve, zh_arp_script_table, zh_arp_span_param, zh_arp_overflows, ZH_ARP_SPAN_FIELDS, kRows, n);
    const zh_script_span_param held[2] = {u1, u2};
    MUST(zh_arp_schedule(arp, 48000.0f, 64, kRows + 1, &in, held) == ZH_ERR_INVALID);
    OK(zh_arp_schedule(arp, 48000.0f, 64, kRows, &in, held));
    OK(zh_arp_overflows(arp, &dropped));
    OK(zh_arp_destroy(arp));

    const uint32_t offsets[2] = {0, 2};
    zh_melody_event ev[2];
    memset(ev, 0, sizeof ev);
    ev[0].note_on = 1; ev[0].note_id = 1; ev[0].freq = 440.0f; ev[1].t = 0.5f; ev[1].note_id = 2; ev[1].freq = 440.0f;
    zh_melody_kit *kit;
    zh_subsong *sub;
    OK(zh_melody_kit_create(c, offsets, 1, ev, 2, &kit));
    OK(zh_subsong_create(c, n, kit, 261.6f, &sub));
    table_pass(sub, zh_subsong_reserve, zh_subsong_script_table, zh_subsong_span_param, zh_subsong_overflows, ZH_SUBSONG_SPAN_FIELDS, kRows, n);
    const zh_script_span_param outer[ZH_SUBSONG_IN_FIELDS] = {f0, u1, u2};
    MUST(zh_subsong_schedule(sub, 48000.0f, 64, kRows + 1, &in, outer) == ZH_ERR_INVALID);
    OK(zh_subsong_schedule(sub, 48000.0f, 64, kRows, &in, outer));
    OK(zh_subsong_overflows(sub, &dropped));
    OK(zh_subsong_destroy(sub));
    OK(zh_melody_kit_destroy(kit));

    zh_span_merge_source src;
    memset(&src, 0, sizeof src);
    src.n_fields = 2; src.on_field = 1; src.kinds[0] = 'f'; src.kinds[1] = 'u';
    zh_span_merge *merge;
    OK(zh_span_merge_create(c, n, &src, &src, &merge));
    table_pass(merge, zh_span_merge_reserve, zh_span_merge_script_table, zh_span_merge_span_param, zh_span_merge_overflows,
               2 + 2 + ZH_SPAN_MERGE_OWN_FIELDS, kRows, n);
    const zh_script_span_param fields[2] = {f0, u1};
    MUST(zh_span_merge_schedule(merge, 64, kRows + 1, &in, fields, &in, fields) == ZH_ERR_INVALID);
    OK(zh_span_merge_schedule(merge, 64, kRows, &in, fields, &in, fields));
    OK(zh_span_merge_overflows(merge, &dropped));
    OK(zh_span_merge_destroy(merge));

    OK(zh_voice_bank_destroy(bank));
    OK(zh_destroy(c));
}

int main(int argc, char **argv) {
    const unsigned rounds = argc > 1 ? (unsigned)atoi(argv[1]) : 300, seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1;
    rs ^= (unsigned long long)seed * 0x9e3779b97f4a7c15ull;
    stage_passes(0);
    stage_passes(5);
    unsigned long paints = 0, captures = 0, launches = 0, refused = 0, held = 0, held_launches = 0;
    for (unsigned round = 0; round < rounds; round++) {
        Ctx cx; cx.capturing = false; cx.flags = 0;
        OK(zh_create(&cx.c, 0));
        OK(zh_malloc(cx.c, (void **)&cx.mix, 64 * 2048 * 4));
        for (unsigned k = 0, n = 1 + pick(4); k < n; k++) add_module(cx);
        for (unsigned step = 0, nsteps = 20 + pick(60); step < nsteps; step++) {
            const unsigned op = pick(100);
            if (cx.capturing) {
                if (op < 70 && !cx.mods.empty()) {                       // a run of paints, mostly of one module (batches form)
                    Mod &m = cx.mods[pick((unsigned)cx.mods.size())];
                    // half of the runs: the same span and flags paint after paint, as a host loop over buffers makes them (batches / the pipeline form)
                    Fixed fx{true, 0, 1024, pick(2), pick(3) != 0, pick(2)};
                    if (!pick(3)) { fx.s = pick(400); fx.e = fx.s + 128 + pick(400); }
                    const bool burst = pick(2) != 0;
                    for (unsigned k = 0, n = 1 + pick(40); k < n; k++) { paint(cx, pick(12) ? m : cx.mods[pick((unsigned)cx.mods.size())], burst ? &fx : nullptr); paints++; }
                } else if (op < 80 && !cx.imgs.empty()) {
                    OK(zh_zero(cx.c, 0, 1024, cx.imgs[pick((unsigned)cx.imgs.size())]));     // another library call between paints: ends the epoch
                } else {
                    zh_graph *g = nullptr;
                    const int rc = zh_graph_end_capture(cx.c, &g);
                    cx.capturing = false;
                    if (rc == ZH_OK) { cx.graphs.push_back(g); unsigned a, b, c2; OK(zh_graph_info(g, &a, &b, &c2)); held += b; held_launches += c2; char kn[512]; OK(zh_graph_kernels(g, kn, sizeof kn)); }
                    else if (rc == ZH_ERR_UNSUPPORTED) refused++;        // a held-back paint that could not be launched after all (deferred error)
                    else { fprintf(stderr, "zh_graph_end_capture -> %d\n", rc); return 1; }
                }
                continue;
            }
            if (op < 25 && !cx.mods.empty()) { paint(cx, cx.mods[pick((unsigned)cx.mods.size())]); paints++; }
            else if (op < 40) { cx.flags = pick(3) ? ZH_CAPTURE_COALESCE : 0; OK(zh_graph_begin_capture_flags(cx.c, cx.flags)); cx.capturing = true; captures++; }
            else if (op < 65 && !cx.graphs.empty()) {
                const int rc = zh_graph_launch(cx.c, cx.graphs[pick((unsigned)cx.graphs.size())]);
                if (rc != ZH_OK && rc != ZH_ERR_INVALID) { fprintf(stderr, "zh_graph_launch -> %d\n", rc); return 1; }   // INVALID: a module of the capture was destroyed since
                launches++;
            }
            else if (op < 72 && !cx.graphs.empty()) { const size_t i = pick((unsigned)cx.graphs.size()); OK(zh_graph_destroy(cx.graphs[i])); cx.graphs.erase(cx.graphs.begin() + (long)i); }
            else if (op < 80 && cx.mods.size() < 6) add_module(cx);
            else if (op < 86 && !cx.mods.empty()) drop_module(cx, pick((unsigned)cx.mods.size()));
            else if (op < 92 && !cx.mods.empty()) {                      // state round trip of a flipper between paints and replays
                Mod &m = cx.mods[pick((unsigned)cx.mods.size())];
                if (m.kind == PULSE) { std::vector<zh_pulseosc_state> st(m.V); OK(zh_pulseosc_get_state((zh_pulseosc *)m.h, st.data())); OK(zh_pulseosc_set_state((zh_pulseosc *)m.h, st.data())); }
                if (m.kind == ENV) { std::vector<zh_envelope_state> st(m.V); OK(zh_envelope_set_state((zh_envelope *)m.h, st.data())); OK(zh_envelope_get_state((zh_envelope *)m.h, st.data())); }
                if (m.kind == DECIM) { std::vector<zh_decimator_state> st(m.V); OK(zh_decimator_set_state((zh_decimator *)m.h, st.data())); OK(zh_decimator_get_state((zh_decimator *)m.h, st.data())); }
                if (m.kind == PMOSC) { std::vector<zh_pmosc_state> st(m.V); OK(zh_pmosc_set_state((zh_pmosc *)m.h, st.data())); OK(zh_pmosc_get_state((zh_pmosc *)m.h, st.data())); }
            }
            else OK(zh_sync(cx.c));
        }
        if (cx.capturing) { zh_graph *g = nullptr; if (zh_graph_end_capture(cx.c, &g) == ZH_OK) cx.graphs.push_back(g); cx.capturing = false; }
        // teardown: modules, then -- half of the time -- the context BEFORE its graphs
        while (!cx.mods.empty()) drop_module(cx, pick((unsigned)cx.mods.size()));
        for (zh_buf &b : cx.imgs) OK(zh_buf_free(cx.c, &b));
        OK(zh_free(cx.c, cx.mix));
        const bool ctx_first = pick(2) != 0;
        if (!ctx_first) for (zh_graph *g : cx.graphs) OK(zh_graph_destroy(g));
        OK(zh_destroy(cx.c));
        if (ctx_first) for (zh_graph *g : cx.graphs) OK(zh_graph_destroy(g));
    }
    unsigned long kl, kc, blocks, graphs, streams;
    hip_stub_report(&kl, &kc, &blocks, &graphs, &streams);
    printf("%u contexts, %lu captures, %lu paints (%lu held back -> %lu launches), %lu replays, %lu captures refused for a deferred error; %lu kernel launches eager + %lu recorded; "
           "left over: %lu device blocks, %lu graphs, %lu streams\n", rounds, captures, paints, held, held_launches, launches, refused, kl, kc, blocks, graphs, streams);
    return (blocks || graphs || streams) ? 2 : 0;
}
