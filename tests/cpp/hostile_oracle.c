/* The hostile-parameter table (tests/hostile_cases.py) through the oracle, as a program of its own: compiled together with
 * oracle/zang_oracle.c under -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all by
 * tests/test_cpp_hostile_oracle.py, so that every tuple and carried state of the table is shown to be DEFINED in the oracle
 * (no overflowing float-to-integer conversion, no out-of-range shift or index) before a device kernel is held to it.
 *
 *     hostile_oracle TABLE RESULTS
 *
 * TABLE (little endian; write_table in tests/hostile_cases.py):
 *     u32 magic "ZHOS", u32 records, u32 frames, u32 spans, then spans x (u32 start, u32 end)
 *     per record: u32 module, u32 vi[6], f32 sample_rate, f32 p[8], u32 note script, u32 has_state, u32 state[12],
 *                 f32 garbage[frames], f32 cin[frames], f32 cctl[frames], f32 cc2[frames]
 * RESULTS: per record f32 out[frames], u32 state[12], f32 further state[1152] (FilteredEchoes: its delay ring; StereoEchoes: the right output, which
 *          starts from cc2, then the rings of the two half delays and of the main delay).
 * The first span is painted with ZERO_FIRST (zo_zero, then the paint) over the garbage, the others add; state is carried. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/zang_oracle.h"

enum { SINE, PULSE, TRISAW, CYCLE, ENVELOPE, PORTAMENTO, DECIMATOR, DISTORTION, FILTER, NICE, PMOSC, ECHOES, CURVE, GATE, SAMPLER, NOISEFILTER, FSAW, HSQUARE,
       STEREO, N_MODULES };
enum { MAX_SPANS = 8, N_SCRIPTS = 5, NST = 12, MAIN_DELAY = 400, NEX = 352 + 2 * MAIN_DELAY, DELAY = 192 };

/* (note_id_changed, note_on) of the four paints: NOTES in tests/hostile_cases.py */
static const int NOTES[N_SCRIPTS][4][2] = {
    {{1, 1}, {0, 1}, {0, 1}, {0, 1}},
    {{1, 1}, {0, 1}, {1, 0}, {0, 0}},
    {{1, 1}, {1, 1}, {0, 1}, {1, 1}},
    {{0, 0}, {0, 0}, {1, 1}, {0, 1}},
    {{0, 0}, {0, 0}, {0, 0}, {0, 0}},
};

static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static zo_cob cob(uint32_t is_image, const float *col, float x) {
    zo_cob c; c.tag = is_image ? ZO_COB_BUFFER : ZO_COB_CONSTANT; c.constant = x; c.buffer = is_image ? col : NULL; return c;
}
static zo_curve curve(uint32_t tag, float d) { zo_curve c; c.tag = tag; c.duration = d; return c; }

static void die(const char *what) { fprintf(stderr, "hostile_oracle: %s\n", what); exit(2); }
static void get(void *dst, size_t n, FILE *f) { if (fread(dst, 1, n, f) != n) die("short table"); }

int main(int argc, char **argv) {
    if (argc != 3) die("usage: hostile_oracle TABLE RESULTS");
    FILE *in = fopen(argv[1], "rb"), *res = fopen(argv[2], "wb");
    if (!in || !res) die("cannot open a file");
    uint32_t head[4], spans[MAX_SPANS][2];
    get(head, sizeof head, in);
    if (head[0] != 0x534F485Au || head[3] != 4 || head[2] == 0 || head[2] > (1u << 20)) die("bad header");
    const uint32_t n = head[1], F = head[2], ns = head[3];
    get(spans, ns * 8, in);
    for (uint32_t i = 0; i < ns; i++) if (spans[i][0] > spans[i][1] || spans[i][1] > F) die("bad span");
    float *out = malloc(F * 4), *cin = malloc(F * 4), *cctl = malloc(F * 4), *cc2 = malloc(F * 4);
    float *t0 = calloc(F, 4), *t1 = calloc(F, 4), *t2 = calloc(F, 4);
    if (!out || !cin || !cctl || !cc2 || !t0 || !t1 || !t2) die("no memory");
    for (uint32_t r = 0; r < n; r++) {
        uint32_t mv[7], kh[2], st[NST], so[NST] = {0};
        float sr, p[8], ring[NEX] = {0};
        get(mv, sizeof mv, in); get(&sr, 4, in); get(p, sizeof p, in); get(kh, sizeof kh, in); get(st, sizeof st, in);
        get(out, F * 4, in); get(cin, F * 4, in); get(cctl, F * 4, in); get(cc2, F * 4, in);
        const uint32_t mid = mv[0], *vi = mv + 1, k = kh[0], has = kh[1];
        if (mid >= N_MODULES || k >= N_SCRIPTS) die("bad record");
        zo_sineosc sine; zo_pulseosc pulse; zo_trisawosc trisaw; zo_cycle cycle; zo_envelope env; zo_portamento port;
        zo_decimator dec; zo_filter flt; zo_nice_instrument nice; zo_pmosc_instrument pm; zo_delay dl; zo_curve_module cv;
        zo_curve_node nodes[64];
        zo_delay d0, d1, de;
        zo_sampler smp; zo_noise nz; zo_filtered_sawtooth fs; zo_hard_square hs; zo_sampler_params sp;
        uint8_t pcm[4096];
        size_t n_nodes = 0;
        zo_sineosc_init(&sine); zo_pulseosc_init(&pulse); zo_trisawosc_init(&trisaw); zo_cycle_init(&cycle); zo_envelope_init(&env);
        zo_portamento_init(&port); zo_decimator_init(&dec); zo_filter_init(&flt);
        zo_nice_init(&nice, p[1]); zo_pmosc_init(&pm, p[1]); zo_delay_init(&dl, ring, DELAY); zo_curve_init(&cv);
        if (mid == STEREO) {
            if (F > 352) die("column too long for the further state");
            memcpy(ring, cc2, F * 4);
            zo_delay_init(&d0, ring + F, MAIN_DELAY / 2); zo_delay_init(&d1, ring + F + MAIN_DELAY / 2, MAIN_DELAY / 2);
            zo_delay_init(&de, ring + F + MAIN_DELAY, MAIN_DELAY);
        }
        zo_sampler_init(&smp); zo_filtered_sawtooth_init(&fs); zo_hard_square_init(&hs);
        zo_noise_init(&nz, (p[7] >= 0.0f && p[7] < 65536.0f) ? (uint64_t)p[7] : 0);      /* NoiseFilter: the voice's seed */
        if (F > sizeof pcm) die("column too long for the sample");
        for (uint32_t j = 0; j < F; j++) pcm[j] = (cc2[j] >= 0.0f && cc2[j] <= 255.0f) ? (uint8_t)cc2[j] : 0;   /* Sampler: mono s16 in cc2 */
        sp.sample_rate = p[0]; sp.num_channels = 1; sp.sample_rate_in = 44100; sp.format = ZO_SAMPLE_S16; sp.data = pcm; sp.data_len = F;
        sp.channel = 0; sp.loop = (int32_t)vi[0];
        if (mid == CURVE) {                                  /* the node list: p[0] (value, t) pairs at the head of cin */
            if (!(p[0] >= 0.0f && p[0] <= 64.0f) || 2 * (uint32_t)p[0] > F) die("bad node count");
            n_nodes = (size_t)p[0];
            for (size_t j = 0; j < n_nodes; j++) { nodes[j].value = cin[2 * j]; nodes[j].t = cin[2 * j + 1]; }
        }
        if (has) {
            sine.t = f_of(st[0]); pulse.cnt = st[0]; trisaw.cnt = st[0]; trisaw.t = f_of(st[1]); cycle.t = f_of(st[0]);
            env.state = st[0]; env.painter.t = f_of(st[1]); env.painter.last_value = f_of(st[2]); env.painter.start = f_of(st[3]);
            port.painter.t = f_of(st[0]); port.painter.last_value = f_of(st[1]); port.painter.start = f_of(st[2]);
            dec.dval = f_of(st[0]); dec.dcount = f_of(st[1]); flt.l = f_of(st[0]); flt.b = f_of(st[1]);
            nice.osc.cnt = st[0]; nice.flt.l = f_of(st[1]); nice.flt.b = f_of(st[2]); nice.env.state = st[3];
            nice.env.painter.t = f_of(st[4]); nice.env.painter.last_value = f_of(st[5]); nice.env.painter.start = f_of(st[6]);
            pm.carrier.t = f_of(st[0]); pm.modulator.t = f_of(st[1]); pm.env.state = st[2];
            pm.env.painter.t = f_of(st[3]); pm.env.painter.last_value = f_of(st[4]); pm.env.painter.start = f_of(st[5]);
            smp.t = f_of(st[0]);
        }
        int prev_on = 0;
        for (uint32_t i = 0; i < ns; i++) {
            const size_t s = spans[i][0], e = spans[i][1];
            const int nic = NOTES[k][i][0], on = NOTES[k][i][1];
            if (i == 0) zo_zero(s, e, out);
            switch (mid) {
            case SINE: zo_sineosc_paint(&sine, s, e, out, sr, cob(vi[0], cctl, p[0]), cob(vi[1], cin, p[1])); break;
            case PULSE: zo_pulseosc_paint(&pulse, s, e, out, sr, cob(vi[0], cctl, p[0]), p[1]); break;
            case TRISAW: zo_trisawosc_paint(&trisaw, s, e, out, sr, cob(vi[0], cctl, p[0]), p[1]); break;
            case CYCLE: zo_cycle_paint(&cycle, s, e, out, sr, cob(vi[0], cctl, p[0])); break;
            case ENVELOPE: {
                zo_envelope_params ep;
                ep.sample_rate = sr; ep.attack = curve(vi[0], p[0]); ep.decay = curve(vi[1], p[1]); ep.release = curve(vi[2], p[2]);
                ep.sustain_volume = p[3]; ep.note_on = on;
                zo_envelope_paint(&env, s, e, out, nic, &ep);
                break;
            }
            case PORTAMENTO: zo_portamento_paint(&port, s, e, out, nic, sr, curve(vi[0], p[0]), p[1], on, prev_on); prev_on = on; break;
            case DECIMATOR: zo_decimator_paint(&dec, s, e, out, sr, cin, p[0]); break;
            case DISTORTION: zo_distortion_paint(s, e, out, cin, vi[0], p[0], p[1], p[2]); break;
            case FILTER: zo_filter_paint(&flt, s, e, out, cin, vi[0], cob(vi[1], cctl, p[0]), cob(vi[2], cc2, p[1])); break;
            case NICE: zo_nice_paint(&nice, s, e, out, t0, t1, nic, sr, p[0], on); break;
            case PMOSC: zo_pmosc_paint(&pm, s, e, out, t0, t1, t2, nic, sr, p[0], on); break;
            case ECHOES: zo_filtered_echoes_paint(&dl, &flt, s, e, out, t0, t1, cin, p[0], p[1]); break;
            case CURVE: zo_curve_paint(&cv, s, e, out, nic, sr, vi[0], nodes, n_nodes); break;
            case STEREO:                                     /* examples/modules.zig:503-522 */
                if (i == 0) zo_zero(s, e, ring);
                zo_add_into(s, e, out, cin); zo_add_into(s, e, ring, cin);
                zo_zero(s, e, t0); zo_simple_delay_paint(&d0, s, e, t0, cin);
                zo_zero(s, e, t1);
                zo_filtered_echoes_paint(&de, &flt, s, e, t1, t2, cctl, t0, p[0], p[1]);   /* (cctl: a column this module does not read, as scratch) */
                zo_add_into(s, e, out, t1);
                zo_simple_delay_paint(&d1, s, e, ring, t1);
                break;
            case GATE: zo_gate_paint(s, e, out, on); break;
            case SAMPLER: zo_sampler_paint(&smp, s, e, out, nic, &sp); break;
            case NOISEFILTER:
                zo_zero(s, e, t0); zo_noise_paint(&nz, s, e, t0, vi[0]);
                zo_filter_paint(&flt, s, e, out, t0, vi[1], cob(0, NULL, p[0]), cob(0, NULL, p[1]));
                break;
            case FSAW: zo_filtered_sawtooth_paint(&fs, s, e, out, t0, t1, t2, nic, sr, cob(vi[0], cctl, p[0]), on); break;
            case HSQUARE: zo_hard_square_paint(&hs, s, e, out, t0, t1, nic, sr, p[0], on); break;
            }
        }
        switch (mid) {
        case SINE: so[0] = u_of(sine.t); break;
        case PULSE: so[0] = pulse.cnt; break;
        case TRISAW: so[0] = trisaw.cnt; so[1] = u_of(trisaw.t); break;
        case CYCLE: so[0] = u_of(cycle.t); break;
        case ENVELOPE: so[0] = env.state; so[1] = u_of(env.painter.t); so[2] = u_of(env.painter.last_value); so[3] = u_of(env.painter.start); break;
        case PORTAMENTO: so[0] = u_of(port.painter.t); so[1] = u_of(port.painter.last_value); so[2] = u_of(port.painter.start); break;
        case DECIMATOR: so[0] = u_of(dec.dval); so[1] = u_of(dec.dcount); break;
        case FILTER: so[0] = u_of(flt.l); so[1] = u_of(flt.b); break;
        case NICE:
            so[0] = nice.osc.cnt; so[1] = u_of(nice.flt.l); so[2] = u_of(nice.flt.b); so[3] = nice.env.state;
            so[4] = u_of(nice.env.painter.t); so[5] = u_of(nice.env.painter.last_value); so[6] = u_of(nice.env.painter.start);
            break;
        case PMOSC:
            so[0] = u_of(pm.carrier.t); so[1] = u_of(pm.modulator.t); so[2] = pm.env.state;
            so[3] = u_of(pm.env.painter.t); so[4] = u_of(pm.env.painter.last_value); so[5] = u_of(pm.env.painter.start);
            break;
        case CURVE:
            so[0] = u_of(cv.t); so[1] = (uint32_t)cv.current_song_note; so[2] = (uint32_t)cv.current_song_note_offset; so[3] = (uint32_t)cv.next_song_note;
            break;
        case STEREO: so[0] = (uint32_t)d0.index; so[1] = (uint32_t)d1.index; so[2] = (uint32_t)de.index; so[3] = u_of(flt.l); so[4] = u_of(flt.b); break;
        case SAMPLER: so[0] = u_of(smp.t); break;
        case NOISEFILTER:
            for (int j = 0; j < 4; j++) { so[2 * j] = (uint32_t)nz.r[j]; so[2 * j + 1] = (uint32_t)(nz.r[j] >> 32); }
            so[8] = u_of(flt.l); so[9] = u_of(flt.b);
            break;
        case ECHOES: so[0] = (uint32_t)dl.index; so[1] = u_of(flt.l); so[2] = u_of(flt.b); break;
        }
        if (mid != ECHOES && mid != STEREO) memset(ring, 0, sizeof ring);
        if (fwrite(out, 4, F, res) != F || fwrite(so, 4, NST, res) != NST || fwrite(ring, 4, NEX, res) != NEX) die("cannot write");
    }
    free(out); free(cin); free(cctl); free(cc2); free(t0); free(t1); free(t2);
    if (fclose(res) != 0) die("cannot write");
    fclose(in);
    printf("%u records PASS\n", n);
    return 0;
}
