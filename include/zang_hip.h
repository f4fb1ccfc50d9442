/* zang_hip.h -- C ABI of libzang_hip.so: zang's module paint() hot path on MI355X (gfx950).
 *
 * The reference (dbandstra/zang, Zig) has no FFI boundary: a module is a Zig struct with
 *     pub fn paint(self, span: zang.Span, outputs: [num_outputs][]f32, temps: [num_temps][]f32,
 *                  note_id_changed: bool, params: Params) void
 * (canonical form: src/modules/SineOsc.zig:8-31; the one type-erased form is
 * ModuleBase.paintFn, src/zangscript/runtime.zig:149-162).  Each `zh_<module>_paint` below
 * replaces that method for a BATCH of n independent voices (= n Zig module instances) in
 * one call; one wavefront lane renders one voice.  Argument order and meaning follow the
 * Zig signature: (self, span.start, span.end, outputs, temps, note_id_changed, params).
 *
 * Sample buffers live in device memory as images laid out [frame][voice] (voice is the
 * fastest index, so the 64 lanes of a wavefront store 256 contiguous bytes per frame).
 * A reference `[]f32` of voice v is column v of an image: element (f, v) = ptr[f*stride + v].
 *
 * Like the reference, every paint ACCUMULATES into outputs[0] (`+=`), and the caller
 * zeroes first (e.g. examples/modules.zig:220-221).  ZH_PAINT_ZERO_FIRST fuses that
 * `zang.zero(span, out)` into the paint kernel (bit-identical to zero-then-paint).  A paint
 * whose input or control image overlaps outputs[0] reads the zeros, as zero-then-paint does:
 * the library then zeroes the span first and paints with ZH_PAINT_ADD.  An image that IS
 * outputs[0] (same pointer and stride) is read in the reference's order: SineOsc, TriSawOsc and
 * Cycle read a frame's control value after they have added to that frame, every other module before.
 *
 * All entry points return 0 on success, a hipError_t (> 0) when HIP failed, or a negative
 * ZH_ERR_* for bad arguments.  Work is enqueued on the context's stream and is
 * asynchronous unless stated; host arrays passed to get/set/upload/download calls are
 * synchronous.  One context per host thread; a module instance must not be painted
 * concurrently (same rule as the reference).  Nothing here allocates inside a paint (the voice
 * mixdown grows a per-context scratch buffer the first time a larger size is needed).  Destroy
 * modules and graphs before their context.
 */
#ifndef ZANG_HIP_H
#define ZANG_HIP_H

#if !defined(__HIPCC_RTC__)   /* hiprtc has no libc headers; it predefines the fixed-width types */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ZH_API __attribute__((visibility("default")))

enum { ZH_OK = 0, ZH_ERR_INVALID = -1, ZH_ERR_UNSUPPORTED = -2, ZH_ERR_NO_DEVICE = -3,
       ZH_ERR_COMM = -4,          /* librccl could not be loaded, or a rendezvous ran out of time (zh_comm_last_error says which) */
       ZH_ERR_RCCL_BASE = -100    /* an RCCL call failed: the code is ZH_ERR_RCCL_BASE - ncclResult_t */ };

/* paint flags */
enum { ZH_PAINT_ADD = 0,         /* out[i] += value          (the reference contract) */
       ZH_PAINT_ZERO_FIRST = 1,  /* zang.zero(span,out) then paint, in one kernel (basics.zig:12) */
       /* (2 = ZH_MIX_SEQUENTIAL, a zh_mixdown_voices flag) */
       ZH_PAINT_PARAMS_UNCHANGED = 4,
       ZH_PAINT_TOLERANT = 8
       /* The caller states that `params` -- scalars AND the contents of every per-voice array -- are what this module's
        * previous paint call was given.  The reference recomputes a paint's per-voice constants on every call
        * (e.g. PulseOsc.zig:87-95); a module may instead reuse the ones that call left behind.  Honoured by the
        * constant-frequency PulseOsc / TriSawOsc paints, ignored elsewhere; results are bit-identical either way.
        * A paint recorded into a graph with this flag uses the constants the module held when it was RECORDED (those of
        * the last unflagged eager paint before the capture): from then on the module stores no new constants -- later
        * unflagged paints compute theirs without keeping them, later flagged paints take the computing form.
        *
        * ZH_PAINT_TOLERANT (opt-in): the caller accepts results within 1e-5 of the signal's peak instead of the reference's bits
        * (north_star: "1e-5 relative f32", bits only for Gate and Decimator).  Honoured by
        *  - zh_filter_paint (constant or control-image cutoff / resonance) and zh_noise_filter_paint (white noise) at up to 16,384 voices,
        *    where the span is then filtered as 32-128-frame chunks at once (csrc/filter_tp.hip.h: zero-state responses, a 2 x 2
        *    transition power, then the reference's own recurrence per chunk; measured error <= 7.3e-6 of the voice's peak over 9,200 random cases,
        *    2.5-3 x faster); the noise samples and generator states are exact, the filter state carries the samples' error;
        *  - zh_nice_paint, zh_nice_paint_mix and zh_nice_paint_mix_stereo at up to 16,384 voices, spans of 128-4,096 frames: the same
        *    for the fused voice's filter (oscillator, envelope and their states exact: the envelope is walked once per voice ahead
        *    of the chunks);
        *  - zh_nice_paint_mix, zh_nice_paint_mix_stereo and zh_nice_paint_mix_stereo_batch ABOVE 16,384 voices: the exact kernel's own
        *    source compiled with multiply-adds fused (csrc/nice_mix_fma.hip: a v_fma_f32 rounds once where the reference rounds
        *    twice; 27 % fewer instructions on a kernel bound by the instructions it issues: 85 against 105 us per buffer at 131,072
        *    voices); phase counters, envelope stages and envelope clocks stay exact; measured error of a mixed sample 1e-3 of the
        *    bound (the sum of the voices' tolerances) over 24 carried buffers;
        *  - zh_noise_paint with ZH_NOISE_PINK at up to 16,384 voices: Kellett's six one-pole taps as chunks at once over exactly
        *    generated white noise (white noise itself, and the generator's state, are always exact);
        *  - zh_sineosc_paint and zh_pmosc_paint (its carrier) at any voice count: the sine of the reference's own rounded
        *    argument in f32 (csrc/zmath.hip.h zsinf_tol: 17 instructions for musl's 34, 15 of them f64; within 4e-7 of it);
        *    phase and envelope states stay exact;
        *  - zh_filtered_echoes_paint at up to 6,144 voices when the span is at most three delay lengths (input image not the
        *    output image): over a piece of <= delay_samples frames the ring's slots were all written before the piece, so the
        *    filter's input is known up front and the piece is filtered as chunks at once (csrc/delay.hip k_fe_tp_a / _b); the
        *    ring carries a paint's error into later ones (measured <= 4.5e-6 of the peak over 200 buffers, feedback 0.9; over 300 further
        *    fuzz seeds of 3-7 carried paints each, 4,096 voices, one voice reached 1.01e-5: profiles/r05/fuzz_long.txt);
        *  - zh_script_module_paint at any voice count: the generated kernel's SineOsc calls and sin() whose result reaches the
        *    output through scaling and adding alone (+ - * neg abs min max, a Filter's or Decimator's input, a delay ring written)
        *    take the f32 sine; one that reaches anything else -- another oscillator's freq or phase, a Distortion, a divisor, pow,
        *    sqrt, sin / cos -- stays exact (csrc/zscript_emit.hip decides per call when the kernel is generated).  The error is
        *    relative to the largest magnitude on the voice's signal path: where large terms cancel it is that of the terms.
        *    (The role-wave form of a generated kernel, zs_paint_pc_<name>, taken at few voices, carries no f32 sine: a tolerant
        *    paint that takes it has the exact bits.)
        * Ignored elsewhere: every other form stays bit-exact, and so does a tolerant Filter paint's first chunk.
        * NO EXCEPTION to the bound (round 5 had one): a voice whose clamped cutoff falls below 2^-9 anywhere in the paint
        * (csrc/filter_tp.hip.h kTpExactCutBelow) is not painted as chunks -- the reference's f32 accumulation of that nearly
        * constant increment drifts systematically from exact arithmetic and a chunked evaluation would depart from it by up to
        * 1.9e-5 of the peak; one lane walks that voice's frames in the reference's own order instead (bit-exact), in the same
        * launch.  Worst over tools/fuzz_tolerant.py's 10,000 seeds: 7.2e-6 of the peak (profiles/r06/fuzz_tolerant_10000.txt).
        * THE BOUND IS PER PAINT, from the state the paint starts on: every sample within 1e-5 of the voice's peak of what the
        * reference paints from that same state.  The filter state a tolerant paint leaves carries the paint's error into the next
        * one.  With damping (a resonance input below 1) that error decays, and a run whose state is carried on the GPU stays
        * inside 1e-5 against the reference carried on its own side (tests/test_gpu_tolerant.py: 200 buffers, Filter / Noise ->
        * Filter / NiceInstrument over config 3's parameter range).  In the undamped corner (resonance input >= 1 clamps the
        * damping to zero, Filter.zig:118) the filter is a lossless resonator and ANY two f32 evaluation orders of its recurrence
        * -- the reference's loop against this library's chunks, or against exact arithmetic -- drift apart like a random walk,
        * ~6e-8 * sqrt(5 * frames) of the state's amplitude (profiles/r05/tolerant_error_floor.txt: chunk start states computed
        * exactly are no closer to the reference than the f32 ones), and a phase difference of a resonator shows as a sample
        * difference that keeps growing: a carried run there departs from the reference by a few 1e-6 of the amplitude per
        * 1,024-frame buffer (tested: within 1e-5 * buffers), whatever form paints it. */ };

typedef struct zh_ctx zh_ctx;

/* Device sample image [frame][voice]; `ptr` is a DEVICE pointer (hipMalloc / torch tensor). */
typedef struct zh_buf {
    float   *ptr;
    uint32_t voices;   /* voices covered by this view                   */
    uint32_t frames;   /* frames (rows) available; spans index into it  */
    uint32_t stride;   /* floats between consecutive frames (>= voices, <= 2^26) */
    uint32_t reserved;
} zh_buf;

/* A per-voice f32 parameter: one value broadcast to every voice, or a device array[n_voices]. */
typedef struct zh_f32 { float value; uint32_t reserved; const float *per_voice; } zh_f32;
/* A per-voice bool parameter (note_on, note_id_changed): broadcast, or device uint8[n_voices]. */
typedef struct zh_bool { uint32_t value; uint32_t reserved; const uint8_t *per_voice; } zh_bool;

/* zang.ConstantOrBuffer (src/zang/constant_or_buffer.zig:4-15).  A buffer is indexed by
 * ABSOLUTE frame ([span.start..span.end], e.g. SineOsc.zig:56). */
enum { ZH_COB_CONSTANT = 0, ZH_COB_BUFFER = 1 };
typedef struct zh_cob { uint32_t tag; uint32_t reserved; zh_f32 constant; zh_buf buffer; } zh_cob;

/* zang.PaintCurve (src/zang/painter.zig:25-30); the tag is shared by all voices. */
enum { ZH_CURVE_INSTANTANEOUS = 0, ZH_CURVE_LINEAR = 1, ZH_CURVE_SQUARED = 2, ZH_CURVE_CUBED = 3 };
typedef struct zh_curve { uint32_t tag; uint32_t reserved; zh_f32 duration; } zh_curve;

/* ---------------------------------------------------------------- context, memory */
ZH_API int  zh_create(zh_ctx **out, int device);
ZH_API int  zh_destroy(zh_ctx *ctx);
ZH_API int  zh_set_stream(zh_ctx *ctx, void *hip_stream);   /* adopt an external hipStream_t; NULL = HIP's default (null) stream.
                                                                 zh_create starts on a private non-blocking stream. */
ZH_API void *zh_get_stream(zh_ctx *ctx);
ZH_API int  zh_sync(zh_ctx *ctx);
ZH_API const char *zh_error_string(int err);
ZH_API const char *zh_version(void);

ZH_API int  zh_malloc(zh_ctx *ctx, void **dev_ptr, size_t bytes);
ZH_API int  zh_free(zh_ctx *ctx, void *dev_ptr);
ZH_API int  zh_upload(zh_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);    /* synchronous */
ZH_API int  zh_download(zh_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);  /* synchronous */

/* out->stride >= voices: rows that would be a multiple of 64 KiB are padded by 4 KiB (HBM bank spreading); always
 * address a sample as ptr[frame * stride + voice]. */
ZH_API int  zh_buf_alloc(zh_ctx *ctx, zh_buf *out, uint32_t voices, uint32_t frames);
ZH_API int  zh_buf_free(zh_ctx *ctx, zh_buf *buf);
/* host image [voice][frame] (one contiguous reference-style []f32 per voice) <-> device [frame][voice] */
ZH_API int  zh_buf_upload_voices(zh_ctx *ctx, zh_buf dst, const float *host_voice_major, uint32_t frames);
ZH_API int  zh_buf_download_voices(zh_ctx *ctx, float *host_voice_major, zh_buf src, uint32_t frames);
/* one voice's []f32 */
ZH_API int  zh_buf_upload_voice(zh_ctx *ctx, zh_buf dst, uint32_t voice, const float *host, uint32_t frames);
ZH_API int  zh_buf_download_voice(zh_ctx *ctx, float *host, zh_buf src, uint32_t voice, uint32_t frames);

/* hipGraph capture of a launch sequence: everything enqueued on the context between begin and
 * end is recorded instead of run; zh_graph_launch replays it with one host call.  A buffer
 * loop (zero + paint + mix per 1024-frame buffer) is launch-bound at small voice counts, and
 * this removes the per-kernel host cost.  (The chunked oscillators double-buffer their phase counters and
 * flip buffers on the host at every paint; the library records which buffer a capture started from and how many
 * flips it holds, and zh_graph_launch copies the live counters over first when eager paints or other graphs
 * have left them in the other buffer -- any number of paints may be captured, and replays and eager paints mix freely.)
 * The voice mixdown's scratch must already be large enough (paint once eagerly first): it cannot grow while
 * a capture is recording (ZH_ERR_UNSUPPORTED).  Destroy a graph BEFORE the context it was captured on (zh_graph_destroy tells the
 * context that one holder of its retired scratch blocks is gone), as with the modules. */
typedef struct zh_graph zh_graph;
ZH_API int  zh_graph_begin_capture(zh_ctx *ctx);
/* The same with flags.  ZH_CAPTURE_COALESCE: the host states that while this capture records, NOTHING but zh_* calls on this
 * context is enqueued on the context's stream.  The library may then hold back paints that depend on nothing recorded before
 * them and record several as one launch: today the constant-frequency zh_pulseosc_paint / zh_trisawosc_paint (and their
 * _batch forms) flagged ZH_PAINT_PARAMS_UNCHANGED -- the reference's loop examples/write_wav.zig:58-66 painting buffer
 * after buffer with unchanged params.  Their phase counter at any frame is the counter at capture entry + frames painted
 * since * ifreq EXACTLY (`cnt +%= ifreq`, PulseOsc.zig:111, TriSawOsc.zig:115), so no paint needs the counters the previous
 * one left: consecutive paints of one module over the same span into images that do not overlap are recorded as ONE
 * launch of up to 32 buffers (exactly the launch zh_pulseosc_paint_batch makes: counters read once, written once).  When
 * something else is recorded, or the capture ends, what is held back goes out.  A capture that recorded NOTHING but such
 * oscillator batches (no other kernel, copy, memset or event, no side stream) is replayed directly: zh_graph_launch enqueues
 * one launch per batch on the context's stream, as zh_pulseosc_paint_batch would -- it reads the live counters and flips, so
 * the 20 paints of one capture are ONE launch of 20 buffers, and no host-side graph launch precedes it (form row
 * `graph_direct`, 1 by default; 0 = always the recorded graph).  The recorded graph stays the fallback: in it the last batch is
 * two launches of half the buffers each where one would leave the module's double-buffered counters on the other side (a
 * replay then ends on the buffer it began on and nothing has to be copied); zh_graph_info describes that graph.  Replays give
 * the same bits as a capture without the flag; what changes is that one launch's ramp and tail are shared by the buffers.
 * Every other call first records what was held back, then itself, in order as before.
 * Also held back: zh_nice_paint_mix_stereo (flagged ZH_PAINT_TOLERANT only from 65,536 voices on).  Its paints DO depend on each other (the voices' state), so
 * they are not reordered: consecutive ones of one instrument over one span with the same gains into different mix rows become the
 * launch zh_nice_paint_mix_stereo_batch makes, up to 8 buffers each -- the state words stay in registers from buffer to buffer and
 * the second pass runs once (105 against 108 us per buffer at 131,072 voices; same bits).  The partial-sum scratch for 8 buffers
 * is reserved by every eager stereo mixdown paint, i.e. by the eager pass a host makes before recording anyway.
 * And PIPELINED: consecutive zh_noise_filter_paint calls flagged ZH_PAINT_TOLERANT (white noise, the two-pass form, one piece each) are
 * recorded so that the second pass of paint n and the first pass of paint n + 1 are ONE launch (the first pass of a paint needs nothing
 * the second pass of the paint before it makes: it starts from the generator state the previous first pass predicted).  16 against
 * 20.5 us per buffer at 4,096 voices; the values are those of the paints recorded one after the other, except that a voice that met one
 * of Random.float's multi-draw samples (2^-41 per sample) is walked sequentially -- the reference's exact walk -- in every later paint
 * of the chain (profiles/r05/probe_overlap_nf.txt).
 * (Measured and rejected, profiles/r05/ab_capture_lanes.txt + ubench_launch_overlap.txt: the same paints as parallel graph
 * branches on 2-4 forked streams -- kernels from different queues slow each other down, 5.0-5.6 against 4.5 us per buffer.) */
enum { ZH_CAPTURE_COALESCE = 1 };
ZH_API int  zh_graph_begin_capture_flags(zh_ctx *ctx, uint32_t flags);
/* how a graph was recorded: nodes in it; paint calls that were held back while recording and the launches they became in the
 * recorded graph (both 0 without ZH_CAPTURE_COALESCE).  A direct replay (ZH_CAPTURE_COALESCE above) may make fewer: zh_graph_kernels */
ZH_API int  zh_graph_info(const zh_graph *graph, uint32_t *nodes, uint32_t *paints_held, uint32_t *launches_of_held);
/* the kernels a replay of the graph runs, in order of first launch while recording, with their counts: "k_osc_const4[batch] x1"
 * (20 paints, replayed directly; "x2" from the recorded graph), "k_nf_tp_a x1,k_nf_tp_ba x19,k_nf_tp_b x1" ([batch]: the
 * instantiation that paints several buffers per launch).  What
 * bench.py's roofline record names: zh_last_form after a paint CALL says nothing about a paint that was held back. */
ZH_API int  zh_graph_kernels(const zh_graph *graph, char *out, size_t n);
ZH_API int  zh_graph_end_capture(zh_ctx *ctx, zh_graph **out);
ZH_API int  zh_graph_launch(zh_ctx *ctx, zh_graph *graph);
ZH_API int  zh_graph_destroy(zh_graph *graph);

/* Which kernel form a paint takes is the library's choice, by voice count, span and arguments.  The voice-count thresholds and
 * frame-range counts behind that choice are ONE table (csrc/dispatch.hip): zh_form_count() rows, zh_form_info(i, ...) = a row's
 * name, default, current value and a line on what it selects and where it was measured.  ZH_FORMS="name=value,name=value" in
 * the environment overrides rows (read once, at the first paint; the parity tests set ZH_ENV_LIVE=1 before loading the library
 * to flip rows between paints).  zh_last_form(ctx, out, n): the kernels launched by the last entry point on this context that
 * launched any, comma-separated in launch order ("k_osc_const4", "k_nf_tp_a,k_nf_tp_b", "k_nice_mix,k_mix_pass2_wide") -- what a host, or bench.py, asks instead of guessing the form from the voice count. */
ZH_API int  zh_form_count(void);
ZH_API int  zh_form_info(int index, const char **name, long *default_value, long *current_value, const char **doc);
ZH_API int  zh_last_form(zh_ctx *ctx, char *out, size_t n);

/* timing helpers: HIP events on the context's stream (used by bench.py) */
typedef struct zh_event zh_event;
ZH_API int  zh_event_create(zh_ctx *ctx, zh_event **out);
ZH_API int  zh_event_destroy(zh_event *ev);
ZH_API int  zh_event_record(zh_ctx *ctx, zh_event *ev);
ZH_API int  zh_event_elapsed_ms(zh_event *start, zh_event *stop, float *ms);  /* synchronises on `stop` */

/* ---------------------------------------------------------------- basics.zig (src/zang/basics.zig:12-78)
 * Each op acts on frames [span_start, span_end) of every voice of `dest`. */
ZH_API int zh_zero(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest);                          /* :12 */
ZH_API int zh_set(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_f32 a);                 /* :16 */
ZH_API int zh_copy(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf src);              /* :20 */
ZH_API int zh_add(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf a, zh_buf b);       /* :24 dest += a+b */
ZH_API int zh_add_into(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf src);          /* :31 */
ZH_API int zh_add_scalar(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf a, zh_f32 b);/* :38 dest += a+b */
ZH_API int zh_add_scalar_into(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_f32 a);     /* :45 */
ZH_API int zh_multiply(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf a, zh_buf b);  /* :52 dest += a*b */
ZH_API int zh_multiply_with(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf a);       /* :59 */
ZH_API int zh_multiply_scalar(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_buf a, zh_f32 b); /* :66 dest += a*b */
ZH_API int zh_multiply_with_scalar(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, zh_buf dest, zh_f32 a);      /* :73 */

/* Voice mixdown: dst[f] += sum over voices of src[f][v], f in the span -- what V successive
 * zang.addInto calls onto one mix buffer do (basics.zig:31-36; example_song.zig:382-396),
 * summed in a FIXED order, so a given (voice count, entry point, row form) always gives the same bits.  `dst` is a device
 * float[frames], added LAST: dst = (ZH_PAINT_ZERO_FIRST ? 0.0f : dst) + total.  The two orders (tests/mix_order_reference.py
 * restates both in numpy float32, and the GPU suite holds every frame to it bit for bit):
 *  - zh_mixdown_voices: tiles of 1,024 voices; lane i of 256 adds its quad ((x0 + x1) + x2) + x3 (a quad cut by the voice count:
 *    0.0f, then += each live voice); a wave's 64 quad sums go through an xor butterfly (32, 16, 8, 4, 2, 1); the four wave sums
 *    of a tile meet in LDS, ((w0 + w1) + w2) + w3.  Second pass: 16 segments of ceil(tiles / 16) consecutive tiles, each a
 *    chain from 0.0f in tile order; total = seg0 + seg1 + ... + seg15.
 *  - zh_nice_paint_mix[_stereo[_batch]]: nothing is shuffled.  Per wave of 64 voices, half h of a frame is the chain x[32h] + x[32h + 1]
 *    + ... + x[32h + 31] (stereo: of the products x * gain, each rounded to f32, never fused; lanes past the last voice add +0.0);
 *    the wave's row is h0 + h1; from 65,536 voices (form row nice_mix_wg_min) the four rows of a workgroup meet in LDS,
 *    ((w0 + w1) + w2) + w3, and one row per 256 voices is written.  Second pass: 128 thread classes, class q a chain from 0.0f
 *    over rows q, q + 128, ...; total = s0 + s1 + ... + s127; the channels are independent.
 * Both second passes start at +0.0f, so a sum of -0.0 voices is +0.0. */
ZH_API int zh_mixdown_voices(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, float *dst, zh_buf src, uint32_t flags);
/* flags for zh_mixdown_voices: ZH_PAINT_ZERO_FIRST, and ZH_MIX_SEQUENTIAL = add voice 0, 1, 2, ... in
 * that order in f32 exactly like successive `+=` paints onto one buffer (example_song.zig:340-346);
 * bit-faithful, meant for small voice counts (one lane per frame walks all voices). */
enum { ZH_MIX_SEQUENTIAL = 2 };

/* ---------------------------------------------------------------- multi-GPU mixdown exchange (new; no reference counterpart)
 * Voices shard across processes, one per GPU; the only data exchanged is each GPU's partial mix.
 * Besides an RCCL all-reduce issued by the host binding, the partials can be written DIRECTLY into the root GPU's
 * memory: the root allocates one slot per rank (zh_ipc_alloc) and passes the 64-byte handle to the other processes
 * by any host channel; they map it (zh_ipc_open) and hand `slot base + rank * slot_bytes` to zh_nice_paint_mix /
 * zh_mixdown_voices as the mix pointer -- the mixdown kernel's stores then travel over xGMI.  When every rank has
 * synchronised its stream (host-side barrier), the root adds the slots in rank order (zh_sum_slots): a fixed
 * order, reproducible bit for bit.  zh_free releases a zh_ipc_alloc block, zh_ipc_close a mapping. */
ZH_API int zh_ipc_alloc(zh_ctx *ctx, size_t bytes, void **dev_ptr, uint8_t *handle64 /* out: 64 bytes */);
ZH_API int zh_ipc_open(zh_ctx *ctx, const uint8_t *handle64, void **dev_ptr);
ZH_API int zh_ipc_close(zh_ctx *ctx, void *dev_ptr);
/* dst[i] (+)= ((slot_0[i] + slot_1[i]) + slot_2[i]) + ... for i < n; slot_r = slots + r * slot_stride_floats.
 * flags: ZH_PAINT_ZERO_FIRST overwrites dst. */
ZH_API int zh_sum_slots(zh_ctx *ctx, float *dst, const float *slots, uint32_t n_slots, size_t slot_stride_floats,
                        size_t n, uint32_t flags);

/* The same exchange as a COLLECTIVE: an RCCL communicator over the GPUs of the node (xGMI), one rank per process, and
 * the partial mixes summed in place on the context's stream, right behind the mixdown kernels that produced them --
 * north_star's "single RCCL reduce over xGMI for the final stereo mixdown".  It replaces the host-side accumulation of
 * the reference's buffer loop (examples/write_wav.zig:58-93: per buffer, every voice paints `+=` into the output
 * channels, then zang.mixDown; examples/example_stereo.zig:84-100 for the two channels), across GPUs.
 * librccl is opened with dlopen on first use (env ZH_RCCL_LIB overrides the search: the copy already in the process,
 * then the sibling of the loaded HIP runtime, then the ROCm installation's).
 *   rank 0:      zh_comm_unique_id(id)  -> hand the 128 bytes to every other process (any host channel)
 *   every rank:  zh_comm_create(ctx, world, rank, id, &comm)     (returns when all `world` ranks have called it, or at the limit)
 *   per batch:   zh_nice_paint_mix[_stereo] ... ; zh_allreduce_mix(comm, mix, n)  or  zh_reduce_mix(..., root)
 * `mix` is a device float[n] of this rank's GPU (e.g. [buffers][channels][frames]); the sum order is RCCL's (ring /
 * tree by size), so unlike zh_sum_slots the bits may differ between world sizes.  Calls on one communicator must be
 * issued in the same order on every rank.  The collectives may be recorded into a graph (zh_graph_begin_capture ...: RCCL
 * supports stream capture), e.g. one per buffer next to the mixdown paints; creating / destroying a communicator may not.  zh_comm_available() = 1 when librccl and its symbols were found.
 * BOUNDED RENDEZVOUS: zh_comm_create meets the other ranks in RCCL's bootstrap.  The communicator is created non-blocking
 * (ncclCommInitRankConfig, blocking = 0) and the calling thread polls ncclCommGetAsyncError; when not every rank has arrived
 * within the limit -- 180 s by default, zh_comm_set_timeout(seconds) or ZH_COMM_TIMEOUT_S in the environment change it,
 * <= 0 = wait for ever -- the half-made communicator is ended with ncclCommAbort and the call returns ZH_ERR_COMM with the
 * reason in zh_comm_last_error().  No helper thread, nothing left behind: the host may retry with a fresh id.
 * It can also return early on ONE rank without entering the bootstrap (ZH_ERR_UNSUPPORTED during a graph capture,
 * ZH_ERR_INVALID for bad arguments / out of memory, ZH_ERR_COMM when librccl is missing): the others then run into the limit.
 * A host that would rather not wait agrees over its own channel BEFORE calling it that every rank (a) sees
 * zh_comm_available() == 1, (b) is not capturing and (c) got the id -- zang_amd.sharding.Comm does exactly that with a MIN
 * all-reduce of the flags; tests/cpp/comm_host.c relies on pipe EOF.
 * AFTER CREATION: zh_comm_check(comm) surfaces ncclCommGetAsyncError -- ZH_OK while nothing is wrong (an operation still in
 * progress is not an error), ZH_ERR_RCCL_BASE - x once a peer died or a transport failed; call it between batches (bench.py
 * does once per timed region).  zh_comm_abort(comm) ends a communicator whose peers may be gone without the collective
 * hand-shake of zh_comm_destroy. */
enum { ZH_COMM_ID_BYTES = 128 };
typedef struct zh_comm zh_comm;
ZH_API int  zh_comm_available(void);
ZH_API const char *zh_comm_library(void);      /* path librccl was opened from ("" if none) */
ZH_API int  zh_comm_version(void);             /* ncclGetVersion, 0 if unavailable */
ZH_API const char *zh_comm_last_error(void);   /* text of this thread's last ZH_ERR_COMM / ZH_ERR_RCCL_BASE-x result */
ZH_API int  zh_comm_unique_id(uint8_t *id128 /* out: ZH_COMM_ID_BYTES */);
ZH_API int  zh_comm_create(zh_ctx *ctx, uint32_t world, uint32_t rank, const uint8_t *id128, zh_comm **out);
ZH_API int  zh_comm_set_timeout(double seconds);   /* process-wide limit of the rendezvous and of calls RCCL answers "in progress" */
ZH_API int  zh_comm_check(zh_comm *comm);
ZH_API int  zh_comm_destroy(zh_comm *comm);    /* synchronises the context's stream first */
ZH_API int  zh_comm_abort(zh_comm *comm);      /* ncclCommAbort: no hand-shake, nothing synchronised */
ZH_API int  zh_comm_world(const zh_comm *comm);
ZH_API int  zh_comm_rank(const zh_comm *comm);
ZH_API int  zh_allreduce_mix(zh_comm *comm, float *mix, size_t n);                 /* every rank ends with the sum */
ZH_API int  zh_reduce_mix(zh_comm *comm, float *mix, size_t n, uint32_t root);     /* only `root` ends with the sum */

/* zang.mixDown (src/zang/mixdown.zig:8-86): f32 mix buffer -> interleaved signed 8 / 16-bit LE PCM with
 * clamping.  `dst` (device bytes, n * bytes_per_sample * num_channels) and `mix` (device float[n]). */
enum { ZH_AUDIO_SIGNED8 = 0, ZH_AUDIO_SIGNED16_LSB = 1 };                                             /* :3-6 */
ZH_API int zh_mix_down(zh_ctx *ctx, uint8_t *dst, const float *mix, uint32_t n, uint32_t audio_format,
                       uint32_t num_channels, uint32_t channel_index, float vol);

/* Grouped voice mixdown: the V voices of `src` are V / group_voices groups of P = group_voices consecutive voices (group g
 * = voices [g*P, (g+1)*P): the sub-voices of instrument g of a voice bank), and every group is mixed on its own.  For each
 * frame f of the span and each group g
 *     s = start value;  s = s + src[f][g*P + 0];  s = s + src[f][g*P + 1];  ...  s = s + src[f][g*P + P-1]
 * in f32, in that order -- the bits of P successive `+=` paints onto one buffer (basics.zig:31-36;
 * example_song.zig:340-346), and of zh_mixdown_voices(ZH_MIX_SEQUENTIAL) on the group's column view -- in ONE launch for
 * all groups, at the rate the image can be read.
 *  - zh_mixdown_groups stores s to dst[g * dst_stride_floats + f].  The start value is +0 with ZH_PAINT_ZERO_FIRST,
 *    otherwise what dst held (`+=`).
 *  - zh_mixdown_groups_pcm passes s through zang.mixDown (mixdown.zig:28-86, exactly zh_mix_down's arithmetic and
 *    rounding) and stores the 1 or 2 bytes at dst[g * dst_stride_bytes + (f * num_channels + channel_index) *
 *    bytes_per_sample]; the other channels' bytes are not touched.  The start value is acc[g * acc_stride_floats + f], or
 *    +0 when acc is NULL.  `acc` chains images: voices of several kinds live in several images, so mix the first into
 *    an f32 row per group, the next ones `+=` onto it, and the last through this call with acc = those rows -- the bits
 *    of one sequential sum over all the sub-voices followed by zh_mix_down.
 * Frames outside the span are neither read nor written.  ZH_ERR_INVALID: a NULL ctx, dst or image; group_voices == 0 or not
 * a divisor of src.voices; span_end < span_start or > src.frames; with more than one group, a stride that does not hold
 * span_end samples; an unknown audio_format, num_channels == 0, channel_index >= num_channels.  ZH_ERR_UNSUPPORTED:
 * ZH_PAINT_TOLERANT.  No groups or an empty span: ZH_OK, nothing is launched.  Neither call synchronises or allocates: both
 * may be recorded into a graph. */
ZH_API int zh_mixdown_groups(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, float *dst, size_t dst_stride_floats,
                             zh_buf src, uint32_t group_voices, uint32_t flags);
ZH_API int zh_mixdown_groups_pcm(zh_ctx *ctx, uint32_t span_start, uint32_t span_end, uint8_t *dst, size_t dst_stride_bytes,
                                 zh_buf src, uint32_t group_voices, const float *acc /* NULL: start from 0 */, size_t acc_stride_floats,
                                 uint32_t audio_format, uint32_t num_channels, uint32_t channel_index, float vol);

/* ---------------------------------------------------------------- SineOsc (src/modules/SineOsc.zig) */
typedef struct zh_sineosc zh_sineosc;
typedef struct zh_sineosc_params { float sample_rate; uint32_t reserved; zh_cob freq; zh_cob phase; } zh_sineosc_params; /* :10-14 */
typedef struct zh_sineosc_state { float t; } zh_sineosc_state;                                        /* :16 */
ZH_API int zh_sineosc_create(zh_ctx *ctx, uint32_t n_voices, zh_sineosc **out);                       /* n x init() :18-22 */
ZH_API int zh_sineosc_destroy(zh_sineosc *m);
ZH_API int zh_sineosc_get_state(zh_sineosc *m, zh_sineosc_state *host);
ZH_API int zh_sineosc_set_state(zh_sineosc *m, const zh_sineosc_state *host);
ZH_API int zh_sineosc_paint(zh_sineosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[1]*/,
                            const zh_buf *temps /*[0]*/, zh_bool note_id_changed,
                            const zh_sineosc_params *params, uint32_t flags);                         /* :24-87 */

/* ---------------------------------------------------------------- PulseOsc (src/modules/PulseOsc.zig) */
typedef struct zh_pulseosc zh_pulseosc;
typedef struct zh_pulseosc_params { float sample_rate; uint32_t reserved; zh_cob freq; zh_f32 color; } zh_pulseosc_params; /* :30-34 */
typedef struct zh_pulseosc_state { uint32_t cnt; } zh_pulseosc_state;                                 /* :36 */
ZH_API int zh_pulseosc_create(zh_ctx *ctx, uint32_t n_voices, zh_pulseosc **out);
ZH_API int zh_pulseosc_destroy(zh_pulseosc *m);
ZH_API int zh_pulseosc_get_state(zh_pulseosc *m, zh_pulseosc_state *host);
ZH_API int zh_pulseosc_set_state(zh_pulseosc *m, const zh_pulseosc_state *host);
ZH_API int zh_pulseosc_paint(zh_pulseosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                             const zh_buf *temps, zh_bool note_id_changed,
                             const zh_pulseosc_params *params, uint32_t flags);                       /* :44-157 */
/* n_buffers consecutive paint calls with the same span and params, buffer b into outputs[b] (what a host loop over
 * 1024-frame buffers does, examples/write_wav.zig:58-66): with a constant frequency the phase counter of any frame is
 * cnt + frames_before * ifreq exactly (:111), so the whole batch is one launch.  State afterwards = after the last call. */
ZH_API int zh_pulseosc_paint_batch(zh_pulseosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[n_buffers]*/,
                                   uint32_t n_buffers, const zh_pulseosc_params *params, uint32_t flags);

/* ---------------------------------------------------------------- TriSawOsc (src/modules/TriSawOsc.zig) */
typedef struct zh_trisawosc zh_trisawosc;
typedef struct zh_trisawosc_params { float sample_rate; uint32_t reserved; zh_cob freq; zh_f32 color; } zh_trisawosc_params; /* :30-34 */
typedef struct zh_trisawosc_state { uint32_t cnt; float t; } zh_trisawosc_state;                      /* :36-37 */
ZH_API int zh_trisawosc_create(zh_ctx *ctx, uint32_t n_voices, zh_trisawosc **out);
ZH_API int zh_trisawosc_destroy(zh_trisawosc *m);
ZH_API int zh_trisawosc_get_state(zh_trisawosc *m, zh_trisawosc_state *host);
ZH_API int zh_trisawosc_set_state(zh_trisawosc *m, const zh_trisawosc_state *host);
ZH_API int zh_trisawosc_paint(zh_trisawosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                              const zh_buf *temps, zh_bool note_id_changed,
                              const zh_trisawosc_params *params, uint32_t flags);                     /* :46-156 */
ZH_API int zh_trisawosc_paint_batch(zh_trisawosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[n_buffers]*/,
                                    uint32_t n_buffers, const zh_trisawosc_params *params, uint32_t flags);   /* see zh_pulseosc_paint_batch */

/* ---------------------------------------------------------------- Noise (src/modules/Noise.zig) */
typedef struct zh_noise zh_noise;
enum { ZH_NOISE_WHITE = 0, ZH_NOISE_PINK = 1 };                                                       /* :11-14 */
typedef struct zh_noise_params { uint32_t color; } zh_noise_params;                                   /* :18-20 */
typedef struct zh_noise_state { uint64_t r[4]; float b[7]; uint32_t reserved; } zh_noise_state;       /* :22-23 */
/* Voice v is seeded like the (first_seed + v)-th Noise.init() of a process (:9,:26): pass the
 * voice's GLOBAL index so that sharded and unsharded renders agree. */
ZH_API int zh_noise_create(zh_ctx *ctx, uint32_t n_voices, uint64_t first_seed, zh_noise **out);
ZH_API int zh_noise_destroy(zh_noise *m);
ZH_API int zh_noise_get_state(zh_noise *m, zh_noise_state *host);
ZH_API int zh_noise_set_state(zh_noise *m, const zh_noise_state *host);
ZH_API int zh_noise_paint(zh_noise *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                          const zh_buf *temps, zh_bool note_id_changed,
                          const zh_noise_params *params, uint32_t flags);                             /* :34-72 */

/* Host-only self-test of the xoshiro256++ jump tables behind the frame-range form of white noise (few voices: a span is
 * painted as many frame ranges at once, each from a state jumped T^(32 j) ahead; csrc/noise_jump.hip): for n_states
 * random states, table j applied to the state must equal 32 (j + 1) sequential transitions, j = 0..62.  Returns the
 * number of mismatching state words (0 = pass).  Needs no device. */
ZH_API int zh_selftest_noise_jump(uint64_t seed, uint32_t n_states);

/* ---------------------------------------------------------------- Envelope (src/modules/Envelope.zig, src/zang/painter.zig) */
typedef struct zh_envelope zh_envelope;
enum { ZH_ENV_IDLE = 0, ZH_ENV_ATTACK, ZH_ENV_DECAY, ZH_ENV_SUSTAIN, ZH_ENV_RELEASE };                /* :15-21 */
typedef struct zh_envelope_params {                                                                   /* :6-13 */
    float sample_rate; uint32_t reserved;
    zh_curve attack, decay, release;
    zh_f32 sustain_volume;
    zh_bool note_on;
} zh_envelope_params;
typedef struct zh_envelope_state { uint32_t state; float t, last_value, start; } zh_envelope_state;   /* :23-24, painter.zig:33-36 */
ZH_API int zh_envelope_create(zh_ctx *ctx, uint32_t n_voices, zh_envelope **out);
ZH_API int zh_envelope_destroy(zh_envelope *m);
ZH_API int zh_envelope_get_state(zh_envelope *m, zh_envelope_state *host);
ZH_API int zh_envelope_set_state(zh_envelope *m, const zh_envelope_state *host);
ZH_API int zh_envelope_paint(zh_envelope *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                             const zh_buf *temps, zh_bool note_id_changed,
                             const zh_envelope_params *params, uint32_t flags);                       /* :92-109 */

/* ---------------------------------------------------------------- Gate (src/modules/Gate.zig) -- stateless */
typedef struct zh_gate zh_gate;
typedef struct zh_gate_params { zh_bool note_on; } zh_gate_params;                                    /* :7-9 */
ZH_API int zh_gate_create(zh_ctx *ctx, uint32_t n_voices, zh_gate **out);
ZH_API int zh_gate_destroy(zh_gate *m);
ZH_API int zh_gate_paint(zh_gate *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                         const zh_buf *temps, zh_bool note_id_changed,
                         const zh_gate_params *params, uint32_t flags);                               /* :15-30 */

/* ---------------------------------------------------------------- Filter (src/modules/Filter.zig) */
typedef struct zh_filter zh_filter;
enum { ZH_FILTER_BYPASS = 0, ZH_FILTER_LOW_PASS, ZH_FILTER_BAND_PASS, ZH_FILTER_HIGH_PASS,
       ZH_FILTER_NOTCH, ZH_FILTER_ALL_PASS };                                                         /* :10-17 */
typedef struct zh_filter_params { zh_buf input; uint32_t type; uint32_t reserved; zh_cob cutoff; zh_cob res; } zh_filter_params; /* :27-32 */
typedef struct zh_filter_state { float l, b; } zh_filter_state;                                       /* :34-35 */
ZH_API int zh_filter_create(zh_ctx *ctx, uint32_t n_voices, zh_filter **out);
ZH_API int zh_filter_destroy(zh_filter *m);
ZH_API int zh_filter_get_state(zh_filter *m, zh_filter_state *host);
ZH_API int zh_filter_set_state(zh_filter *m, const zh_filter_state *host);
ZH_API int zh_filter_paint(zh_filter *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                           const zh_buf *temps, zh_bool note_id_changed,
                           const zh_filter_params *params, uint32_t flags);                           /* :44-151 */
/* Filter.cutoffFromFrequency (:20-23) for n values, on the device (host scalar in the reference). */
ZH_API int zh_filter_cutoff_from_frequency(zh_ctx *ctx, uint32_t n, float *cutoff_out_dev,
                                           const float *frequency_dev, float sample_rate);

/* std.math.pow(f32, x, y) for finite x > 0, elementwise on the device (out, x, y: device float[n]).
 * Host callers of the paint path compute scalars with it: note frequencies a4 * pow(2, semitones/12)
 * (examples/common/songparse1.zig:61-62), Distortion's gain1 (Distortion.zig:41). */
ZH_API int zh_pow(zh_ctx *ctx, uint32_t n, float *out, const float *x, const float *y);
/* std.math.sin / std.math.cos (f32), elementwise on the device for any float (inf and nan included): the
 * functions SineOsc (SineOsc.zig:4-6), PMOscInstrument and Filter.cutoffFromFrequency (Filter.zig:21) are
 * built on, exposed so that a host can compute its scalars with the same bits (out, x: device float[n]). */
ZH_API int zh_sin(zh_ctx *ctx, uint32_t n, float *out, const float *x);
ZH_API int zh_cos(zh_ctx *ctx, uint32_t n, float *out, const float *x);
/* std.math.atan (f32), the function of Distortion's overdrive (Distortion.zig:45, 50), same contract. */
ZH_API int zh_atan(zh_ctx *ctx, uint32_t n, float *out, const float *x);

/* ---------------------------------------------------------------- Sampler (src/modules/Sampler.zig) */
typedef struct zh_sampler zh_sampler;
enum { ZH_SAMPLE_U8 = 0, ZH_SAMPLE_S16_LSB, ZH_SAMPLE_S24_LSB, ZH_SAMPLE_S32_LSB };                   /* :9-14 */
typedef struct zh_sample {                                                                            /* :16-21 */
    uint64_t num_channels; uint64_t sample_rate; uint32_t format; uint32_t reserved;
    const uint8_t *data;   /* DEVICE pointer to the PCM bytes, shared read-only by all voices */
    uint64_t data_len;     /* bytes */
} zh_sample;
typedef struct zh_sampler_params {                                                                    /* :62-67 */
    zh_f32 sample_rate;    /* per-voice: example_sampler.zig varies it per note to change pitch */
    zh_sample sample; uint64_t channel; uint32_t loop; uint32_t reserved;
} zh_sampler_params;
typedef struct zh_sampler_state { float t; } zh_sampler_state;                                        /* :69 */
ZH_API int zh_sampler_create(zh_ctx *ctx, uint32_t n_voices, zh_sampler **out);
ZH_API int zh_sampler_destroy(zh_sampler *m);
ZH_API int zh_sampler_get_state(zh_sampler *m, zh_sampler_state *host);
ZH_API int zh_sampler_set_state(zh_sampler *m, const zh_sampler_state *host);
ZH_API int zh_sampler_paint(zh_sampler *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                            const zh_buf *temps, zh_bool note_id_changed,
                            const zh_sampler_params *params, uint32_t flags);                         /* :77-136 */

/* A sample kit: K samples resident on the device, each with its own format, channel count, native rate and length (a drum
 * machine's or a multi-sampled instrument's recordings: every Sampler instance of the reference holds its own Sample, and the
 * sample is a Params field, Sampler.zig:62-67, so every note may pick another: examples/example_sampler.zig:86-91, :123-138).
 * zh_sample_kit_create is THE ONE PLACE where zh_sample.data is read as a HOST pointer: the PCM bytes of samples[0..n) are
 * copied into one device blob owned by the kit (every sample at a 4-byte-aligned offset; bytes after a sample's last whole
 * frame are kept: they count in data_len for the wrap of :133-135 and are never decoded), with a descriptor table beside it.
 * The call synchronises and is not capturable; the caller's arrays may be freed on return.  data_len == 0 is a valid, silent
 * sample.  ZH_ERR_INVALID: n == 0, a format above ZH_SAMPLE_S32_LSB, num_channels == 0, data == NULL with data_len > 0, more
 * than INT32_MAX frames (the reference's @intCast(i32, ...) traps, :42).  Destroy a kit after the last paint that reads it has
 * run, and before its context.
 * zh_sample_kit_sample fills a zh_sample whose `data` is the DEVICE pointer of entry i (valid while the kit lives): what
 * zh_sampler_paint / zh_sampler_paint_spans take to play one entry of a kit. */
typedef struct zh_sample_kit zh_sample_kit;
ZH_API int zh_sample_kit_create(zh_ctx *ctx, const zh_sample *samples, uint32_t n, zh_sample_kit **out);
ZH_API int zh_sample_kit_destroy(zh_sample_kit *kit);
ZH_API int zh_sample_kit_count(const zh_sample_kit *kit, uint32_t *count_out);
ZH_API int zh_sample_kit_sample(const zh_sample_kit *kit, uint32_t i, zh_sample *out);

/* ---------------------------------------------------------------- Decimator (src/modules/Decimator.zig) */
typedef struct zh_decimator zh_decimator;
typedef struct zh_decimator_params { float sample_rate; uint32_t reserved; zh_buf input; zh_f32 fake_sample_rate; } zh_decimator_params; /* :5-9 */
typedef struct zh_decimator_state { float dval, dcount; } zh_decimator_state;                         /* :11-12 */
ZH_API int zh_decimator_create(zh_ctx *ctx, uint32_t n_voices, zh_decimator **out);
ZH_API int zh_decimator_destroy(zh_decimator *m);
ZH_API int zh_decimator_get_state(zh_decimator *m, zh_decimator_state *host);
ZH_API int zh_decimator_set_state(zh_decimator *m, const zh_decimator_state *host);
ZH_API int zh_decimator_paint(zh_decimator *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                              const zh_buf *temps, zh_bool note_id_changed,
                              const zh_decimator_params *params, uint32_t flags);                     /* :21-57 */

/* The decimated group mix: the bus of examples/example_polyphony.zig (:135-163) for every group at once, ONE kernel.  `m` is a
 * Decimator of one voice per GROUP of `src` (groups as in zh_mixdown_groups: group g = voices [g*P, (g+1)*P), P = group_voices);
 * its get_state / set_state are the groups' Decimator states.  For every group g and every frame f of the span
 *     mix = +0 + src[f][g*P + 0] + ... + src[f][g*P + P-1]       in f32, in that order: the bits of zh_mixdown_groups with
 *                                                                 ZH_PAINT_ZERO_FIRST (the zeroed temps[2], :135)
 * and then, onto the row dst[g * dst_stride_floats + f] (start value +0 with ZH_PAINT_ZERO_FIRST, otherwise what dst held):
 *  - modes[g].bypass != 0:             dst = start + mix (addInto, :162); the Decimator's state is not touched;
 *  - otherwise exactly Decimator.paint (src/modules/Decimator.zig:34-56) with input = mix, fake_sample_rate =
 *    modes[g].fake_sample_rate: fake >= sample_rate: dst = start + mix, then the state is reset to dval = 0, dcount = 1;
 *    fake > 0: the hold (dcount += fake / sample_rate; at dcount >= 1 dval = mix and dcount -= 1; dst = start + dval); anything
 *    else (zero, negative, NaN): nothing is added and the state is not touched (with ZH_PAINT_ZERO_FIRST the span is +0).
 *    The comparisons and the quotient are the reference's, so a non-finite rate does what it does there.
 * Frames outside the span are neither read nor written.  `modes` is device memory, [groups], read by the kernel.  Return codes
 * and the cases where nothing is launched (no groups, an empty span -- the state is then not reset either) are those of
 * zh_mixdown_groups; also ZH_ERR_INVALID: a NULL m or modes, m's voice count != src.voices / group_voices.  ZH_ERR_UNSUPPORTED:
 * ZH_PAINT_TOLERANT.  No sync, no allocation: capturable.  The state is updated in place (no flip of the double buffer). */
typedef struct zh_group_decimation { float fake_sample_rate; uint32_t bypass; } zh_group_decimation;
ZH_API int zh_decimator_paint_groups(zh_decimator *m /* n_voices == number of groups */, uint32_t span_start, uint32_t span_end,
                                     float *dst, size_t dst_stride_floats, zh_buf src, uint32_t group_voices, float sample_rate,
                                     const zh_group_decimation *modes /* device [groups] */, uint32_t flags);

/* ---------------------------------------------------------------- Distortion (src/modules/Distortion.zig) -- stateless */
typedef struct zh_distortion zh_distortion;
enum { ZH_DISTORTION_OVERDRIVE = 0, ZH_DISTORTION_CLIP = 1 };                                         /* :8-11 */
typedef struct zh_distortion_params { zh_buf input; uint32_t type; uint32_t reserved; zh_f32 ingain, outgain, offset; } zh_distortion_params; /* :15-21 */
ZH_API int zh_distortion_create(zh_ctx *ctx, uint32_t n_voices, zh_distortion **out);
ZH_API int zh_distortion_destroy(zh_distortion *m);
ZH_API int zh_distortion_paint(zh_distortion *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                               const zh_buf *temps, zh_bool note_id_changed,
                               const zh_distortion_params *params, uint32_t flags);                   /* :27-66 */

/* ---------------------------------------------------------------- Curve (src/modules/Curve.zig)
 * (entry points are named zh_curve_module_* because zh_curve is zang.PaintCurve)
 * Node times may be any f32: a time becomes a frame through the saturating conversion (NaN -> 0) and is only ever compared with
 * frames of the span, never used as an address; where the difference of two such frames leaves i32 (a checked-arithmetic panic
 * in the reference) it wraps.
 * The node carried over from the previous paint is read at the index that paint left (current_song_note), whatever curve_len is
 * now: do not pass a shorter node list without note_id_changed (which restarts at node 0). */
typedef struct zh_curve_module zh_curve_module;
enum { ZH_CURVE_FN_LINEAR = 0, ZH_CURVE_FN_SMOOTHSTEP = 1 };                                          /* :4-7 */
typedef struct zh_curve_node { float value, t; } zh_curve_node;                                       /* zang.CurveNode, src/zang/curve.zig:3-6 */
typedef struct zh_curve_module_params {                                                               /* :29-33 */
    float sample_rate; uint32_t function;
    const zh_curve_node *curve;   /* DEVICE array shared by all voices (must not be mutated while painting, :37-38) */
    uint64_t curve_len;
} zh_curve_module_params;
typedef struct zh_curve_module_state {                                                                /* :36-41 */
    float t; uint32_t current_song_note; int32_t current_song_note_offset; uint32_t next_song_note;
} zh_curve_module_state;
ZH_API int zh_curve_module_create(zh_ctx *ctx, uint32_t n_voices, zh_curve_module **out);
ZH_API int zh_curve_module_destroy(zh_curve_module *m);
ZH_API int zh_curve_module_get_state(zh_curve_module *m, zh_curve_module_state *host);
ZH_API int zh_curve_module_set_state(zh_curve_module *m, const zh_curve_module_state *host);
ZH_API int zh_curve_module_paint(zh_curve_module *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                                 const zh_buf *temps, zh_bool note_id_changed,
                                 const zh_curve_module_params *params, uint32_t flags);               /* :56-128 */

/* ---------------------------------------------------------------- Cycle (src/modules/Cycle.zig) */
typedef struct zh_cycle zh_cycle;
typedef struct zh_cycle_params { float sample_rate; uint32_t reserved; zh_cob speed; } zh_cycle_params;          /* :9-12 */
typedef struct zh_cycle_state { float t; } zh_cycle_state;                                            /* :14 */
ZH_API int zh_cycle_create(zh_ctx *ctx, uint32_t n_voices, zh_cycle **out);
ZH_API int zh_cycle_destroy(zh_cycle *m);
ZH_API int zh_cycle_get_state(zh_cycle *m, zh_cycle_state *host);
ZH_API int zh_cycle_set_state(zh_cycle *m, const zh_cycle_state *host);
ZH_API int zh_cycle_paint(zh_cycle *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                          const zh_buf *temps, zh_bool note_id_changed,
                          const zh_cycle_params *params, uint32_t flags);                             /* :22-59 */

/* ---------------------------------------------------------------- Portamento (src/modules/Portamento.zig) */
typedef struct zh_portamento zh_portamento;
typedef struct zh_portamento_params {                                                                 /* :5-11 */
    float sample_rate; uint32_t reserved; zh_curve curve; zh_f32 goal; zh_bool note_on; zh_bool prev_note_on;
} zh_portamento_params;
typedef struct zh_portamento_state { float t, last_value, start; } zh_portamento_state;               /* :13, painter.zig:33-36 */
ZH_API int zh_portamento_create(zh_ctx *ctx, uint32_t n_voices, zh_portamento **out);
ZH_API int zh_portamento_destroy(zh_portamento *m);
ZH_API int zh_portamento_get_state(zh_portamento *m, zh_portamento_state *host);
ZH_API int zh_portamento_set_state(zh_portamento *m, const zh_portamento_state *host);
ZH_API int zh_portamento_paint(zh_portamento *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                               const zh_buf *temps, zh_bool note_id_changed,
                               const zh_portamento_params *params, uint32_t flags);                   /* :21-48 */

/* ---------------------------------------------------------------- NiceInstrument (examples/modules.zig:189-248)
 * PulseOsc -> x0.5 -> Filter(low_pass, cutoffFromFrequency(8*freq), res 0.7) -> Envelope(cubed
 * .01/.1/.5, sustain .8) -> out += env*flt, as ONE kernel: the two temps never touch HBM. */
typedef struct zh_nice zh_nice;
typedef struct zh_nice_params { float sample_rate; uint32_t reserved; zh_f32 freq; zh_bool note_on; } zh_nice_params; /* :192-196 */
typedef struct zh_nice_state { zh_pulseosc_state osc; zh_filter_state flt; zh_envelope_state env; } zh_nice_state;    /* :198-201 */
ZH_API int zh_nice_create(zh_ctx *ctx, uint32_t n_voices, zh_f32 color, zh_nice **out);               /* init(color) :203-210 */
ZH_API int zh_nice_destroy(zh_nice *m);
ZH_API int zh_nice_get_state(zh_nice *m, zh_nice_state *host);
ZH_API int zh_nice_set_state(zh_nice *m, const zh_nice_state *host);
ZH_API int zh_nice_paint(zh_nice *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                         const zh_buf *temps /*[2], unused by the fused kernel; may be NULL*/,
                         zh_bool note_id_changed, const zh_nice_params *params, uint32_t flags);      /* :212-247 */
/* The same chain, then the voice mixdown, without materialising per-voice output:
 * partial[f] (+)= sum_v voice_v[f].  `mix` is a device float[frames]. */
ZH_API int zh_nice_paint_mix(zh_nice *m, uint32_t span_start, uint32_t span_end, float *mix,
                             zh_bool note_id_changed, const zh_nice_params *params, uint32_t flags);
/* Two output channels (a module with num_outputs = 2, examples/example_stereo.zig:42-43): every voice is added to each
 * channel scaled by that voice's channel gain, `outputs[c] += voice * pan_c` (example_stereo.zig:92-98, zang.multiply:
 * product rounded to f32, then added), and each channel is mixed down over the voices:
 * mix_c[f] (+)= sum_v voice_v[f] * gain_c[v].  mix_left / mix_right are device float[frames] (zh_mix_down then
 * interleaves them, examples/write_wav.zig:71-78). */
ZH_API int zh_nice_paint_mix_stereo(zh_nice *m, uint32_t span_start, uint32_t span_end, float *mix_left, float *mix_right,
                                    zh_f32 gain_left, zh_f32 gain_right, zh_bool note_id_changed,
                                    const zh_nice_params *params, uint32_t flags);

/* n_buffers consecutive zh_nice_paint_mix_stereo calls -- the host's loop over 1024-frame buffers (examples/write_wav.zig:58-93)
 * of an offline render that knows its params ahead -- as ONE launch: buffer b paints [span_start, span_end) with params[b] and
 * note_id_changed[b] into mix_left[b] / mix_right[b] (host arrays of n_buffers device pointers / structs); the voices' state
 * stays in registers from buffer to buffer and the second mixdown pass runs once for all buffers.  Bit-identical to n_buffers
 * single calls; the sample rate must be the same in every params[b] (ZH_ERR_UNSUPPORTED otherwise). */
/* Scratch: the fused mixdown keeps per-context partial rows in HBM -- frames (rounded up to 8) x rows x channels x 4 bytes per
 * buffer, rows = one per 256 voices from 65,536 voices up and one per 64 voices below (ZH_NICE_MIX_WG_MIN): 4 MiB per stereo
 * buffer of 1,024 frames at 131,072 voices, 32 MiB at 1,048,576; a batch reserves n_buffers times that (512 MiB for 16 buffers at
 * 1 Mi voices).  The block only grows, on the first call that needs more (never inside a capture: ZH_ERR_UNSUPPORTED -- make one
 * eager call of the size first); an outgrown block is freed at once unless a captured graph of the context is alive, then when
 * the last one is destroyed. */
enum { ZH_MIX_MAX_BATCH = 16 };
ZH_API int zh_nice_paint_mix_stereo_batch(zh_nice *m, uint32_t span_start, uint32_t span_end, uint32_t n_buffers,
                                          float *const *mix_left, float *const *mix_right, zh_f32 gain_left, zh_f32 gain_right,
                                          const zh_bool *note_id_changed, const zh_nice_params *params, uint32_t flags);

/* Per-voice span table: the output of NoteTracker -> PolyphonyDispatcher -> Trigger for one buffer
 * (examples/example_song.zig:326-349), i.e. for every voice up to `max_spans` sub-spans, ascending and
 * non-overlapping, each with the note's params and note_id_changed.  One launch then performs, per voice,
 * the same sequence of paint(sub_span, ..., note_id_changed, params) calls the reference's Trigger loop
 * makes (per-call prologue/epilogue included).  With more than 64 voices a lane owns a voice and the wave walks
 * segments between sub-span boundaries; with up to 64 voices a WAVE owns a voice and its lanes are 64 consecutive
 * frames (only what truly carries state from frame to frame -- phase and envelope clocks, the filter core -- is
 * walked frame by frame; oscillator, envelope curve and sines are evaluated for 64 frames at once) -- the same
 * values either way.  Arrays are device memory laid out [span_index][voice]; zh_poly_voice_schedule fills this layout. */
typedef struct zh_span_table {
    uint32_t max_spans, reserved;
    const uint32_t *count;                       /* [n_voices]            */
    const uint32_t *start, *end;                 /* [max_spans][n_voices] */
    const float    *freq;                        /* [max_spans][n_voices] */
    const uint8_t  *note_on, *note_id_changed;   /* [max_spans][n_voices] */
} zh_span_table;
ZH_API int zh_nice_paint_spans(zh_nice *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                               const zh_buf *temps, float sample_rate, const zh_span_table *table, uint32_t flags);

/* ---------------------------------------------------------------- Delay(n) and its composites
 * zang.Delay(delay_samples) (src/zang/delay.zig:7-91) is a per-voice ring buffer; on the device the rings of
 * n voices form one image [delay_sample][voice] in HBM.  Two modules use it:
 *   zh_delay           = SimpleDelay   (examples/modules.zig:341-386): out += ring; ring = input
 *   zh_filtered_echoes = FilteredEchoes (examples/modules.zig:390-461): feedback*ring + input -> low-pass -> out, ring
 * The reference moves data in chunks of <= delay_samples (read, then write); reading a slot always precedes
 * writing it, so the per-sample form used by the kernels is equivalent.  StereoEchoes (:463-525) is zh_stereo_echoes
 * below: the same composition as one kernel. */
typedef struct zh_delay zh_delay;
typedef struct zh_delay_params { zh_buf input; } zh_delay_params;                                     /* :345-347 */
ZH_API int zh_delay_create(zh_ctx *ctx, uint32_t n_voices, uint32_t delay_samples, zh_delay **out);   /* init(): ring zeros, index 0 */
ZH_API int zh_delay_destroy(zh_delay *m);
ZH_API int zh_delay_reset(zh_delay *m);                                                               /* delay.zig:19-22 */
/* state: host float[n_voices][delay_samples] (one ring per voice) and uint32 index[n_voices] */
ZH_API int zh_delay_get_state(zh_delay *m, float *rings_voice_major, uint32_t *index);
ZH_API int zh_delay_set_state(zh_delay *m, const float *rings_voice_major, const uint32_t *index);
ZH_API int zh_delay_paint(zh_delay *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                          const zh_buf *temps, zh_bool note_id_changed, const zh_delay_params *params, uint32_t flags);

typedef struct zh_filtered_echoes zh_filtered_echoes;
typedef struct zh_filtered_echoes_params { zh_buf input; zh_f32 feedback_volume; zh_f32 cutoff; } zh_filtered_echoes_params; /* :394-398 */
ZH_API int zh_filtered_echoes_create(zh_ctx *ctx, uint32_t n_voices, uint32_t delay_samples, zh_filtered_echoes **out);
ZH_API int zh_filtered_echoes_destroy(zh_filtered_echoes *m);
ZH_API int zh_filtered_echoes_reset(zh_filtered_echoes *m);                                           /* :407-409: the delay only */
ZH_API int zh_filtered_echoes_get_state(zh_filtered_echoes *m, float *rings_voice_major, uint32_t *index, zh_filter_state *filter);
ZH_API int zh_filtered_echoes_set_state(zh_filtered_echoes *m, const float *rings_voice_major, const uint32_t *index, const zh_filter_state *filter);
ZH_API int zh_filtered_echoes_paint(zh_filtered_echoes *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                                    const zh_buf *temps /*[2], unused; may be NULL*/, zh_bool note_id_changed,
                                    const zh_filtered_echoes_params *params, uint32_t flags);

/* ---------------------------------------------------------------- StereoEchoes(MAIN_DELAY) (examples/modules.zig:464-525)
 * The bus effect of example_delay.zig / example_detuned.zig as ONE kernel: the dry input into both outputs, SimpleDelay(HALF)
 * into a zeroed temp, FilteredEchoes(MAIN) on that temp, its output into the left channel and through a second SimpleDelay(HALF)
 * into the right; HALF = main_delay / 2 (:465).  Per frame, in the reference's order of f32 operations:
 *   L += x; R += x; t0 = 0 + ring0; ring0 = x; t1 = FilteredEchoes' frame on (ring_e, t0); ring_e = t1;
 *   L += 0 + t1; R += ring1; ring1 = 0 + t1
 * Bit-identical to the composition of the calls above.  State per voice: the rings delay0 and delay1 (HALF samples), the ring
 * echoes (MAIN samples) with its filter (l, b), and one index per ring.  reset() clears the three delays, not the filter
 * (:488-492, :408-410).  get_state / set_state take each ring as zh_delay_get_state does; an index that is not below its ring's
 * length is ZH_ERR_INVALID.
 * paint: outputs[0] = left, outputs[1] = right; the four temps of the reference are not needed.  ZH_PAINT_ZERO_FIRST starts both
 * outputs from +0 without reading them.  Images may be views (any stride >= n_voices, any 4-byte aligned base).  No two of input,
 * outputs[0] and outputs[1] may share memory: ZH_ERR_INVALID (column ranges of one allocation with one stride do not; views of
 * different strides whose extents intersect count as sharing).  main_delay < 2 is ZH_ERR_INVALID at create; ZH_PAINT_TOLERANT is
 * ZH_ERR_UNSUPPORTED.  A paint neither allocates nor synchronises.  Up to the table's stereo_echoes_pc_max voices with main_delay >= 192
 * and a span of at least 64 frames: loader / filter / writer waves per 64 voices (k_stereo_echoes_pc); otherwise one lane per
 * voice (k_stereo_echoes). */
typedef struct zh_stereo_echoes zh_stereo_echoes;
typedef struct zh_stereo_echoes_params { zh_buf input; zh_f32 feedback_volume; zh_f32 cutoff; } zh_stereo_echoes_params;   /* :470-474 */
ZH_API int zh_stereo_echoes_create(zh_ctx *ctx, uint32_t n_voices, uint32_t main_delay, zh_stereo_echoes **out);
ZH_API int zh_stereo_echoes_destroy(zh_stereo_echoes *m);
ZH_API int zh_stereo_echoes_reset(zh_stereo_echoes *m);
ZH_API int zh_stereo_echoes_get_state(zh_stereo_echoes *m, float *rings0_voice_major, uint32_t *index0, float *rings1_voice_major, uint32_t *index1,
                                      float *rings_e_voice_major, uint32_t *index_e, zh_filter_state *filter);
ZH_API int zh_stereo_echoes_set_state(zh_stereo_echoes *m, const float *rings0_voice_major, const uint32_t *index0, const float *rings1_voice_major,
                                      const uint32_t *index1, const float *rings_e_voice_major, const uint32_t *index_e, const zh_filter_state *filter);
ZH_API int zh_stereo_echoes_paint(zh_stereo_echoes *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                                  const zh_buf *temps /*[4], unused; may be NULL*/, zh_bool note_id_changed,
                                  const zh_stereo_echoes_params *params, uint32_t flags);

/* ---------------------------------------------------------------- Noise -> Filter voice (examples/example_stereo.zig:71-82)
 * zero(temp); Noise.paint(temp); Filter.paint(out, input = temp, type, cutoff, res) as ONE kernel: the
 * temp image stays in registers (BASELINE config 3, fused variant).  Bit-identical to the two separate
 * paints.  cutoff / res are per-voice constants here. */
typedef struct zh_noise_filter zh_noise_filter;
typedef struct zh_noise_filter_params { uint32_t color; uint32_t type; zh_f32 cutoff; zh_f32 res; } zh_noise_filter_params;
typedef struct zh_noise_filter_state { zh_noise_state noise; zh_filter_state flt; } zh_noise_filter_state;
ZH_API int zh_noise_filter_create(zh_ctx *ctx, uint32_t n_voices, uint64_t first_seed, zh_noise_filter **out);
ZH_API int zh_noise_filter_destroy(zh_noise_filter *m);
ZH_API int zh_noise_filter_get_state(zh_noise_filter *m, zh_noise_filter_state *host);
ZH_API int zh_noise_filter_set_state(zh_noise_filter *m, const zh_noise_filter_state *host);
ZH_API int zh_noise_filter_paint(zh_noise_filter *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                                 const zh_buf *temps /*[1], unused; may be NULL*/, zh_bool note_id_changed,
                                 const zh_noise_filter_params *params, uint32_t flags);

/* ---------------------------------------------------------------- PMOscInstrument (examples/modules.zig:6-128) */
typedef struct zh_pmosc zh_pmosc;
typedef struct zh_pmosc_params { float sample_rate; uint32_t reserved; zh_f32 freq; zh_bool note_on; } zh_pmosc_params; /* :83-87 */
typedef struct zh_pmosc_state { zh_sineosc_state carrier, modulator; zh_envelope_state env; } zh_pmosc_state;          /* :24-25, :89-91 */
ZH_API int zh_pmosc_create(zh_ctx *ctx, uint32_t n_voices, zh_f32 release_duration, zh_pmosc **out);  /* init(release_duration) :93-99 */
ZH_API int zh_pmosc_destroy(zh_pmosc *m);
ZH_API int zh_pmosc_get_state(zh_pmosc *m, zh_pmosc_state *host);
ZH_API int zh_pmosc_set_state(zh_pmosc *m, const zh_pmosc_state *host);
ZH_API int zh_pmosc_paint(zh_pmosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                          const zh_buf *temps /*[3], unused; may be NULL*/,
                          zh_bool note_id_changed, const zh_pmosc_params *params, uint32_t flags);    /* :101-127 */
ZH_API int zh_pmosc_paint_spans(zh_pmosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                                const zh_buf *temps, float sample_rate, const zh_span_table *table, uint32_t flags);

/* ---------------------------------------------------------------- FM synth voice (examples/example_fmsynth.zig:22-356)
 * The OPL-style two-operator instrument as ONE kernel: Instrument (:244-356) = modulator + carrier Operator (:92-242), each an
 * Oscillator (:26-89: four waveforms, its own last two samples fed back into its phase) times volume, tremolo and an Envelope
 * with cubed curves.  Algorithm 0 adds both operators into the output, modulator first; algorithm 1 makes the modulator the
 * carrier's phase.  Bit-identical to the reference's stage-by-stage composition.
 * `group` consecutive voices form one INSTRUMENT (a synth's polyphony): instrument j = voice / group selects the patch and the
 * column of the two LFO images, which hold one column per instrument ([frame][ceil(n_voices / group)]) and are read at the
 * absolute frame.  A patch is the 22 discrete parameters of :375-398; zh_fm_set_patches turns them into gains and envelope times
 * once (:135-203), on the device, and a paint only loads its instrument's numbers.  Waveform, algorithm and feedback are
 * per voice at run time: voices with different patches share a launch.
 * ZH_FM_SPLIT_OPERATORS (these two paints only): outputs[0] has 2 * n_voices columns; column 2v receives what voice v's modulator
 * adds to the output (nothing in algorithm 1), column 2v + 1 what its carrier adds.  The reference's synth adds every voice into
 * ONE buffer, (acc + m_v) + c_v (:462, :302, :335), which in f32 is not acc + (m_v + c_v): zh_mixdown_groups over groups of
 * 2 * group columns of the split image reproduces that order.  Without the flag a voice's column is its own paint, (out + m) + c.
 * ZH_ERR_INVALID: NULL or mis-sized images (outputs[0]: n_voices or 2 * n_voices columns; the LFO images: one per instrument), a
 * span outside an image, group == 0, a bad table, a patch value outside its num_values (nothing changes then), n_patches neither
 * 1 nor the number of instruments.  ZH_ERR_UNSUPPORTED: ZH_PAINT_TOLERANT (exact forms only); zh_fm_set_patches while a capture
 * records (it copies from the host).  Both paints are capturable; neither allocates nor synchronises. */
enum { ZH_FM_MOD_FREQ_MUL = 0, ZH_FM_MOD_WAVEFORM = 1, ZH_FM_MOD_VOLUME = 2, ZH_FM_MOD_ATTACK = 3, ZH_FM_MOD_DECAY = 4,
       ZH_FM_MOD_SUSTAIN = 5, ZH_FM_MOD_RELEASE = 6, ZH_FM_MOD_TREMOLO = 7, ZH_FM_MOD_VIBRATO = 8, ZH_FM_MOD_FEEDBACK = 9,
       ZH_FM_CAR_FREQ_MUL = 10, ZH_FM_CAR_WAVEFORM = 11, ZH_FM_CAR_VOLUME = 12, ZH_FM_CAR_ATTACK = 13, ZH_FM_CAR_DECAY = 14,
       ZH_FM_CAR_SUSTAIN = 15, ZH_FM_CAR_RELEASE = 16, ZH_FM_CAR_TREMOLO = 17, ZH_FM_CAR_VIBRATO = 18, ZH_FM_TREMOLO_DEPTH = 19,
       ZH_FM_VIBRATO_DEPTH = 20, ZH_FM_ALGORITHM = 21, ZH_FM_PATCH_VALUES = 22 };   /* the order of parameters[0..21], :375-398 */
enum { ZH_FM_SPLIT_OPERATORS = 16 };   /* a paint flag beside ZH_PAINT_*: zh_fm_paint and zh_fm_paint_spans only */
typedef struct zh_fm zh_fm;
typedef struct zh_fm_patch { uint32_t value[22]; } zh_fm_patch;                /* [ZH_FM_PATCH_VALUES]: current_value, :376-397 */
typedef struct zh_fm_params { float sample_rate; uint32_t reserved; zh_buf tremolo_input, vibrato_input; zh_f32 freq; zh_bool note_on; } zh_fm_params; /* :247-275 */
typedef struct zh_fm_op_state { float t, feedback1, feedback2; uint32_t reserved; zh_envelope_state env; } zh_fm_op_state;   /* :37-39, :116-117 */
typedef struct zh_fm_state { zh_fm_op_state modulator, carrier; } zh_fm_state;                         /* :277-278 */
ZH_API int zh_fm_patch_default(zh_fm_patch *patch);                                                    /* the current_values of :376-397 */
ZH_API int zh_fm_create(zh_ctx *ctx, uint32_t n_voices, uint32_t group, zh_fm **out);                  /* init() :280-285, default patch */
ZH_API int zh_fm_destroy(zh_fm *m);
ZH_API int zh_fm_set_patches(zh_fm *m, const zh_fm_patch *patches, uint32_t n_patches);                /* :135-203, once instead of per paint */
ZH_API int zh_fm_get_state(zh_fm *m, zh_fm_state *host);
ZH_API int zh_fm_set_state(zh_fm *m, const zh_fm_state *host);
ZH_API int zh_fm_paint(zh_fm *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                       const zh_buf *temps /*[3], unused; may be NULL*/,
                       zh_bool note_id_changed, const zh_fm_params *params, uint32_t flags);           /* :287-355 */
ZH_API int zh_fm_paint_spans(zh_fm *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                             const zh_buf *temps, float sample_rate, zh_buf tremolo_input, zh_buf vibrato_input,
                             const zh_span_table *table, uint32_t flags);                               /* the Trigger loop :457-496; freq / note_on = NoteParams :365-368 */

/* ---------------------------------------------------------------- zangscript modules
 * The reference compiles its module DSL to Zig source (tools/zangc.zig -> src/zangscript/codegen_zig.zig) that is
 * then built into the host program.  Here the same front-end (python -m zang_amd.zangc, zang_amd/zangscript/)
 * emits HIP source with ONE fused lane-per-voice kernel per exported module -- every temp buffer of the
 * generated Zig paint() becomes a per-frame register -- and this loader compiles it for gfx950 with hiprtc
 * and runs it.  The call shape stays the module contract of SineOsc.zig:8-31: paint(span, outputs, temps,
 * note_id_changed, params), with the script module's Params (codegen_zig.zig:520-527) passed as an array of
 * zh_script_param in declaration order (index 0 is the implicit `sample_rate`, parse.zig:330-331). */
enum { ZH_SP_CONSTANT = 0,   /* f32: `f`, or `pf` per voice                                         */
       ZH_SP_BOOLEAN = 1,    /* bool: `u`, or `pb` per voice                                        */
       ZH_SP_COB = 2,        /* zang.ConstantOrBuffer: is_buffer ? image pf/stride : constant f|pf   */
       ZH_SP_BUFFER = 3,     /* []const f32 ("waveform"): image pf/stride                           */
       ZH_SP_ENUM = 4,       /* one_of: `u` = index of the value in the enum's declaration order,
                                `f` = its f32 payload if it has one (PaintCurve durations)          */
       ZH_SP_CURVE = 5 };    /* []const zang.CurveNode: pf = DEVICE zh_curve_node array, u = count  */
typedef struct zh_script_param {
    uint32_t kind, u;
    float f;
    uint32_t is_buffer;
    const float *pf;
    const uint8_t *pb;
    uint32_t stride, reserved;
} zh_script_param;
#define ZH_SCRIPT_MAX_PARAMS 16

typedef struct zh_script zh_script;                 /* one compiled + loaded script (a hipModule) */
typedef struct zh_script_module zh_script_module;   /* n_voices instances of one exported module */
/* Compile only (no GPU needed): returns a malloc'ed gfx950 code object, or the compiler log in `log`. */
ZH_API int zh_script_compile(const char *hip_source, void **code_out, size_t *code_size_out, char *log, size_t log_cap);
ZH_API void zh_script_free_code(void *code);
ZH_API int zh_script_load(zh_ctx *ctx, const char *hip_source, zh_script **out, char *log, size_t log_cap);
/* ... or from the code object zh_script_compile returned earlier -- compiled once, offline (hiprtc needs no GPU), like the reference
 * compiles a script to Zig before the program is built (examples/example_script.zig:6-8): no hiprtc at run time (1-4 s per module). */
ZH_API int zh_script_load_code(zh_ctx *ctx, const void *code, size_t code_size, zh_script **out);
ZH_API int zh_script_destroy(zh_script *s);
/* `name` = the exported module's global name; `state_words` = 32-bit state words per voice as reported by the
 * front-end; Noise fields are seeded first_seed + voice * n_noise_fields + k (Noise.zig:25-29: one counter tick
 * per init(), instances created voice by voice). */
ZH_API int zh_script_module_create(zh_script *s, const char *name, uint32_t n_voices, uint32_t state_words,
                                   uint64_t first_seed, zh_script_module **out);
ZH_API int zh_script_module_destroy(zh_script_module *m);
/* 1 when this module's kernel may be launched as frame ranges at small voice counts (its frame body writes no memory: no
 * delay ring), 0 otherwise */
ZH_API int zh_script_module_ranges_ok(zh_script_module *m);
ZH_API int zh_script_module_get_state(zh_script_module *m, uint32_t *host_words);         /* [word][voice] */
ZH_API int zh_script_module_set_state(zh_script_module *m, const uint32_t *host_words);
ZH_API int zh_script_module_paint(zh_script_module *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                                  zh_bool note_id_changed, const zh_script_param *params, uint32_t n_params, uint32_t flags);
/* Per-voice sub-spans of a module for one buffer: what NoteTracker -> PolyphonyDispatcher -> Trigger yields
 * (examples/example_script_runtime_poly.zig:146-164).  Device arrays [span_index][voice], like zh_span_table.  Taken by
 * zh_script_module_paint_spans and by the builtin modules' zh_<module>_paint_spans (below), with zh_script_span_param. */
typedef struct zh_script_span_table {
    uint32_t max_spans, reserved;
    const uint32_t *count;            /* [n_voices]                 */
    const uint32_t *start, *end;      /* [max_spans][n_voices]      */
    const uint8_t  *note_id_changed;  /* [max_spans][n_voices]      */
} zh_script_span_table;
/* Per-sub-span values of param i ([max_spans][n_voices] device arrays).  Both NULL: params[i] holds for every sub-span.
 * (zh_<module>_paint_spans: of span field i, ZH_<MODULE>_SPAN_*.) */
typedef struct zh_script_span_param {
    const float    *f;   /* ZH_SP_CONSTANT, the constant of a ZH_SP_COB, the f32 payload of a ZH_SP_ENUM */
    const uint32_t *u;   /* ZH_SP_BOOLEAN (0/1), the index of a ZH_SP_ENUM */
} zh_script_span_param;
/* zh_zscript_generate_hip_forms: next to zs_paint_<name>, zs_paint_spans_<name> (zh_script_module_paint_spans) */
#define ZH_ZSCRIPT_FORM_SPANS 8
/* One launch does, for every voice v, the reference's sequence of paint(sub_span_k, outputs, temps, note_id_changed[k][v],
 * params_k) calls for k < min(count[v], max_spans), each call's prologue and epilogue included, empty sub-spans (start == end)
 * at any position too.  Sub-spans of a voice are ascending and non-overlapping inside [span_start, span_end]; a sub-span that
 * starts before the previous one ends, or before span_start, is never reached and ends the voice's list.  Frames of a voice
 * that no sub-span covers are left as they are; with ZH_PAINT_ZERO_FIRST every frame of [span_start, span_end) is written, 0
 * where nothing paints.  params[i] keeps its zh_script_module_paint meaning wherever span_params[i] (host array [n_params], or
 * NULL for none) gives no array; waveform images and cob images stay indexed by absolute frame, curves stay shared.
 * ZH_ERR_UNSUPPORTED: the module was generated without ZH_ZSCRIPT_FORM_SPANS, or ZH_PAINT_TOLERANT is set (the form is exact
 * only).  ZH_ERR_INVALID: a span array on a BUFFER or CURVE param or on a COB param whose is_buffer is set, `u` on a CONSTANT or
 * COB, `f` on a BOOLEAN, a NULL table array, max_spans == 0.  No voices: ZH_OK, nothing runs.  Capturable (no host sync). */
ZH_API int zh_script_module_paint_spans(zh_script_module *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                                        const zh_script_param *params, uint32_t n_params, const zh_script_span_param *span_params,
                                        const zh_script_span_table *table, uint32_t flags);

/* ---------------------------------------------------------------- the builtin modules over per-voice sub-span tables
 * A polyphonic voice paints its modules through Trigger: one paint(sub_span, outputs, temps, note_id_changed, params) per
 * sub-span with that note's Params (src/zang/trigger.zig:80-105; examples/example_polyphony.zig:81-90,
 * example_sampler.zig:96-105, example_song.zig:336-347).  zh_<module>_paint_spans does that for every voice of a module
 * object in one launch, with the semantics of zh_script_module_paint_spans above: for each voice v and k < min(count[v],
 * max_spans), paint(sub_span_k, ..., note_id_changed[k][v], params_k), each call's prologue and epilogue included, empty
 * sub-spans too; a sub-span out of order ends the voice's list; frames no sub-span covers are left alone, ZH_PAINT_ZERO_FIRST
 * writes all of [span_start, span_end).  span_params (NULL = none) is a host array [ZH_<MODULE>_SPAN_FIELDS]: entry i gives
 * field i per sub-span (`f` float, `u` uint32 device arrays [max_spans][n_voices]).  A field without an array keeps its
 * zh_<module>_paint meaning: a broadcast value, a per-voice array, or a cob buffer / input image read at the ABSOLUTE frame.
 * The scalar sample_rate of the oscillators, Envelope and Decimator, the Sampler's sample and channel and the Noise seeds
 * stay shared.  Tags in span arrays are not checked (out of range: unspecified output, no memory access outside the arguments).
 * ZH_ERR_INVALID: NULL params, a NULL table array or max_spans == 0, `f` on a `u`-only field or `u` on an `f`-only field,
 * a span array on a cob whose tag is ZH_COB_BUFFER, a tag out of range in params; ZH_ERR_UNSUPPORTED: ZH_PAINT_TOLERANT
 * (the form is exact only).  ZH_PAINT_PARAMS_UNCHANGED is ignored: the form neither reads nor stores the constants it lets a
 * PulseOsc / TriSawOsc paint reuse, and it counts as that module's previous paint -- the next flagged zh_<osc>_paint
 * recomputes its constants.  No voices: ZH_OK, nothing runs.  No host sync: capturable; under ZH_CAPTURE_COALESCE it records what was held
 * back first.  Module state follows the plain paints' bookkeeping, so span paints, plain paints and graph replays mix.
 * The overlap rules at the top of this header hold for the span forms (zh_script_module_paint_spans too): a ZH_PAINT_ZERO_FIRST
 * paint whose input or control image overlaps outputs[0] reads the zeros -- the library zeroes the span, then paints with
 * ZH_PAINT_ADD -- and an image that IS outputs[0] is read in the reference's order (SineOsc and TriSawOsc read a frame's
 * frequency after their own add to that frame, every other image is read before it). */
enum { ZH_SINEOSC_SPAN_FREQ = 0,          /* f (a constant freq only) */
       ZH_SINEOSC_SPAN_PHASE,             /* f (a constant phase only) */
       ZH_SINEOSC_SPAN_FIELDS };
enum { ZH_PULSEOSC_SPAN_FREQ = 0,         /* f (a constant freq only) */
       ZH_PULSEOSC_SPAN_COLOR,            /* f */
       ZH_PULSEOSC_SPAN_FIELDS };
enum { ZH_TRISAWOSC_SPAN_FREQ = 0,        /* f (a constant freq only) */
       ZH_TRISAWOSC_SPAN_COLOR,           /* f */
       ZH_TRISAWOSC_SPAN_FIELDS };
enum { ZH_NOISE_SPAN_COLOR = 0,           /* u */
       ZH_NOISE_SPAN_FIELDS };
enum { ZH_ENVELOPE_SPAN_ATTACK = 0,       /* u = curve tag, f = duration */
       ZH_ENVELOPE_SPAN_DECAY,            /* u = curve tag, f = duration */
       ZH_ENVELOPE_SPAN_RELEASE,          /* u = curve tag, f = duration */
       ZH_ENVELOPE_SPAN_SUSTAIN_VOLUME,   /* f */
       ZH_ENVELOPE_SPAN_NOTE_ON,          /* u (0 / non-zero) */
       ZH_ENVELOPE_SPAN_FIELDS };
enum { ZH_GATE_SPAN_NOTE_ON = 0,          /* u (0 / non-zero) */
       ZH_GATE_SPAN_FIELDS };
enum { ZH_FILTER_SPAN_TYPE = 0,           /* u */
       ZH_FILTER_SPAN_CUTOFF,             /* f (a constant cutoff only) */
       ZH_FILTER_SPAN_RES,                /* f (a constant res only) */
       ZH_FILTER_SPAN_FIELDS };
enum { ZH_SAMPLER_SPAN_SAMPLE_RATE = 0,   /* f (negative: backwards, examples/example_sampler.zig:131-137) */
       ZH_SAMPLER_SPAN_LOOP,              /* u (0 / non-zero) */
       ZH_SAMPLER_SPAN_FIELDS };
enum { ZH_DECIMATOR_SPAN_FAKE_SAMPLE_RATE = 0,   /* f */
       ZH_DECIMATOR_SPAN_FIELDS };
enum { ZH_DISTORTION_SPAN_TYPE = 0,       /* u */
       ZH_DISTORTION_SPAN_INGAIN,         /* f */
       ZH_DISTORTION_SPAN_OUTGAIN,        /* f */
       ZH_DISTORTION_SPAN_OFFSET,         /* f */
       ZH_DISTORTION_SPAN_FIELDS };
ZH_API int zh_sineosc_paint_spans(zh_sineosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                  const zh_sineosc_params *params, const zh_script_span_param *span_params /*[ZH_SINEOSC_SPAN_FIELDS]*/,
                                  const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_pulseosc_paint_spans(zh_pulseosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                   const zh_pulseosc_params *params, const zh_script_span_param *span_params /*[ZH_PULSEOSC_SPAN_FIELDS]*/,
                                   const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_trisawosc_paint_spans(zh_trisawosc *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                    const zh_trisawosc_params *params, const zh_script_span_param *span_params /*[ZH_TRISAWOSC_SPAN_FIELDS]*/,
                                    const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_noise_paint_spans(zh_noise *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                const zh_noise_params *params, const zh_script_span_param *span_params /*[ZH_NOISE_SPAN_FIELDS]*/,
                                const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_envelope_paint_spans(zh_envelope *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                   const zh_envelope_params *params, const zh_script_span_param *span_params /*[ZH_ENVELOPE_SPAN_FIELDS]*/,
                                   const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_gate_paint_spans(zh_gate *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                               const zh_gate_params *params, const zh_script_span_param *span_params /*[ZH_GATE_SPAN_FIELDS]*/,
                               const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_filter_paint_spans(zh_filter *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                 const zh_filter_params *params, const zh_script_span_param *span_params /*[ZH_FILTER_SPAN_FIELDS]*/,
                                 const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_sampler_paint_spans(zh_sampler *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                  const zh_sampler_params *params, const zh_script_span_param *span_params /*[ZH_SAMPLER_SPAN_FIELDS]*/,
                                  const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_decimator_paint_spans(zh_decimator *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                    const zh_decimator_params *params, const zh_script_span_param *span_params /*[ZH_DECIMATOR_SPAN_FIELDS]*/,
                                    const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_distortion_paint_spans(zh_distortion *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                     const zh_distortion_params *params, const zh_script_span_param *span_params /*[ZH_DISTORTION_SPAN_FIELDS]*/,
                                     const zh_script_span_table *table, uint32_t flags);

/* The Sampler over a SAMPLE KIT: the sample and the channel are per-note values like every other Params field
 * (Sampler.zig:62-67).  zh_sampler_paint_kit_spans is zh_sampler_paint_spans with two more span fields: for each voice v and
 * k < min(count[v], max_spans), paint(sub_span_k, ..., note_id_changed[k][v], {sample_rate, kit[sample], channel, loop}_k) as
 * the reference's Trigger loop hands each sub-span the sample of its own note (examples/example_sampler.zig:96-105), in one
 * launch (k_sampler_kit_spans): each lane reads the descriptor of its own sample, the PCM format is a run-time value of the
 * lane, and lanes of one wave take the plain (:105-114) and the resampling (:116-130) path at once.  The contract is that of
 * the zh_<module>_paint_spans above -- empty sub-spans run their prologue, a sub-span out of order ends the voice's list,
 * ZH_PAINT_ZERO_FIRST writes all of [span_start, span_end), ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED, no host sync: capturable --
 * except that NOTHING of the Sampler stays shared but the kit itself (one kit per call).  A field without a span array takes
 * its value from `params`: a broadcast value or a per-voice device array.  Per sub-span, in the reference's order: channel >=
 * the sample's num_channels paints nothing and leaves `t` alone, EVEN WHEN note_id_changed is set (:87-89 come before :91-93);
 * a sample index >= the kit's count is DEFINED the same way (nothing painted, the state untouched, no memory read); then the
 * reset of `t`, ratio = sample.sample_rate / sample_rate, the return for a negative ratio without loop, and the wrap by
 * data.len in BYTES when looping (:133-135).  A sub-span may play another sample than the one before it with note_id_changed
 * clear: `t` carries over, as in the reference.  State is the zh_sampler's `t` with the plain paints' bookkeeping: kit
 * paints, plain paints, span paints and graph replays of one zh_sampler mix.
 * zh_sampler_paint_kit is the uniform-span form: n Sampler instances, each with its own sample, channel, rate and loop flag,
 * painting [span_start, span_end) in one launch of the same kernel.
 * ZH_ERR_INVALID: what zh_<module>_paint_spans refuses, a NULL kit, a kit of another context, an output image that is NULL or
 * too small. */
typedef struct zh_u32 { uint32_t value; uint32_t reserved; const uint32_t *per_voice; } zh_u32;   /* broadcast, or device uint32[n_voices] */
typedef struct zh_sampler_kit_params {
    zh_f32 sample_rate;    /* the output rate (pitch; negative: backwards, examples/example_sampler.zig:131-137) */
    zh_bool loop;
    zh_u32 sample;         /* index into the kit */
    zh_u32 channel;
    const zh_sample_kit *kit;
} zh_sampler_kit_params;
enum { ZH_SAMPLER_KIT_SPAN_SAMPLE_RATE = 0,   /* f */
       ZH_SAMPLER_KIT_SPAN_LOOP,              /* u (0 / non-zero) */
       ZH_SAMPLER_KIT_SPAN_SAMPLE,            /* u */
       ZH_SAMPLER_KIT_SPAN_CHANNEL,           /* u */
       ZH_SAMPLER_KIT_SPAN_FIELDS };
ZH_API int zh_sampler_paint_kit_spans(zh_sampler *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                      const zh_sampler_kit_params *params, const zh_script_span_param *span_params /*[ZH_SAMPLER_KIT_SPAN_FIELDS]*/,
                                      const zh_script_span_table *table, uint32_t flags);
ZH_API int zh_sampler_paint_kit(zh_sampler *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                zh_bool note_id_changed, const zh_sampler_kit_params *params, uint32_t flags);

/* ---------------------------------------------------------------- sound-effect voice (examples/example_laser.zig:22-117)
 * LaserPlayer as ONE kernel: three Curves (modulator frequency, carrier frequency, volume) drive a phase-modulated pair of
 * SineOscs; a one-shot effect fired by an impulse, no note-off.  Bit-identical to the reference's stage order, per sub-span
 * (Cm, Cc, Cv = the effect's curves, i = a frame of the sub-span):
 *   f_m[i] = (0 + Cm(i)) * (freq_mul * modulator_mul)      (the scalar product rounded once per paint; the `0 +` is zang.zero
 *                                                           followed by Curve's `+=`; a frame the curve does not paint is +0.0)
 *   p[i]   = (0 + sin((t_m + 0) * pi * 2)) * modulator_rad;  t_m += f_m[i] * (1 / sample_rate)     (SineOsc.zig:62-75)
 *   f_c[i] = (0 + Cc(i)) * (freq_mul * carrier_mul)
 *   c[i]   = 0 + sin((t_c + p[i]) * pi * 2);                 t_c += f_c[i] * (1 / sample_rate)     (SineOsc.zig:76-85)
 *   out[i] += (0 + Cv(i)) * c[i]                            (multiply, round, add: never fused; on EVERY frame of the sub-span)
 * and after the sub-span t_m -= trunc(t_m), t_c -= trunc(t_c).
 * An EFFECT KIT (zh_sfx_kit) holds K effects, each three node lists (any length, 0 too) with their own interpolation function:
 * all nodes concatenated in one device array beside a descriptor table.  The reference hard-wires one triple and gets its four
 * sounds from the four scalars (:161-220); here the effect index is a per-note value beside them.  zh_sfx_kit_create is THE ONE
 * PLACE where zh_sfx_curve.nodes is read as a HOST pointer; it synchronises and is not capturable.  zh_sfx_kit_effect fills a
 * zh_sfx_effect whose `nodes` are DEVICE pointers (valid while the kit lives): what zh_curve_module_params.curve takes, to paint
 * an effect stage by stage.  zh_sfx_effect_default fills in the reference's triple (:22-38; nodes[0..2] modulator, [3..5]
 * carrier, [6..8] volume, all smoothstep).  ZH_ERR_INVALID: n == 0, nodes == NULL with count > 0, a function outside
 * ZH_CURVE_FN_*; nothing is created then.  Destroy a kit after the last paint that reads it has run, and before its context.
 * Each curve behaves exactly as zh_curve_module_paint does for the same node list, function, sample rate, note_id_changed and
 * sub-span length (hostile node times and the at-most-32 span nodes per paint included).  As there, the node carried over from
 * the previous paint is read at the index that paint left (current_song_note), counted from the first node of the curve the
 * sub-span plays NOW: when the effect changes without note_id_changed, that is whichever node of the kit's array lies there
 * (the array ends with as many zero nodes as the kit's longest curve has, so the read stays inside it; an index that only
 * zh_laser_set_state can produce, past the array, drops the carried node).  An effect index >= the kit's count is DEFINED:
 * nothing is painted, none of the five states changes, no node is read -- even when note_id_changed is set.
 * zh_laser_paint_spans is the Trigger loop of :149-158 for every voice in one launch, with the contract of
 * zh_sampler_paint_kit_spans: empty sub-spans run their prologue, a sub-span out of order ends the voice's list,
 * ZH_PAINT_ZERO_FIRST writes all of [span_start, span_end), ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED; a field without a span
 * array takes its value from `params` (a broadcast value or a per-voice device array).  Neither paint allocates or
 * synchronises: both are capturable, and paints, span paints and graph replays of one zh_laser mix.
 * ZH_ERR_INVALID: what zh_<module>_paint_spans refuses, a NULL kit, a kit of another context, an output image that is NULL or
 * too small. */
typedef struct zh_sfx_kit zh_sfx_kit;
typedef struct zh_sfx_curve { const zh_curve_node *nodes; uint32_t count; uint32_t function; } zh_sfx_curve;   /* function: ZH_CURVE_FN_* */
typedef struct zh_sfx_effect { zh_sfx_curve modulator, carrier, volume; } zh_sfx_effect;               /* :22-38, in paint order */
ZH_API int zh_sfx_effect_default(zh_sfx_effect *effect, zh_curve_node *nodes /*[9]: what the effect's curves point at*/);
ZH_API int zh_sfx_kit_create(zh_ctx *ctx, const zh_sfx_effect *effects, uint32_t n, zh_sfx_kit **out);
ZH_API int zh_sfx_kit_destroy(zh_sfx_kit *kit);
ZH_API int zh_sfx_kit_count(const zh_sfx_kit *kit, uint32_t *count_out);
ZH_API int zh_sfx_kit_effect(const zh_sfx_kit *kit, uint32_t i, zh_sfx_effect *out);
typedef struct zh_laser zh_laser;
typedef struct zh_laser_params {                                                                       /* :43-49 */
    float sample_rate; uint32_t reserved;
    zh_f32 freq_mul, carrier_mul, modulator_mul, modulator_rad;
    zh_u32 effect;         /* index into the kit */
    const zh_sfx_kit *kit;
} zh_laser_params;
typedef struct zh_laser_state {                                                                        /* :51-55 */
    zh_curve_module_state carrier_curve; zh_sineosc_state carrier;
    zh_curve_module_state modulator_curve; zh_sineosc_state modulator;
    zh_curve_module_state volume_curve;
} zh_laser_state;
enum { ZH_LASER_SPAN_FREQ_MUL = 0,        /* f */
       ZH_LASER_SPAN_CARRIER_MUL,         /* f */
       ZH_LASER_SPAN_MODULATOR_MUL,       /* f */
       ZH_LASER_SPAN_MODULATOR_RAD,       /* f */
       ZH_LASER_SPAN_EFFECT,              /* u */
       ZH_LASER_SPAN_FIELDS };
ZH_API int zh_laser_create(zh_ctx *ctx, uint32_t n_voices, zh_laser **out);                            /* init() :57-65 */
ZH_API int zh_laser_destroy(zh_laser *m);
ZH_API int zh_laser_get_state(zh_laser *m, zh_laser_state *host);
ZH_API int zh_laser_set_state(zh_laser *m, const zh_laser_state *host);
ZH_API int zh_laser_paint(zh_laser *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs,
                          const zh_buf *temps /*[3], unused; may be NULL*/,
                          zh_bool note_id_changed, const zh_laser_params *params, uint32_t flags);     /* :67-116 */
ZH_API int zh_laser_paint_spans(zh_laser *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs, const zh_buf *temps,
                                const zh_laser_params *params, const zh_script_span_param *span_params /*[ZH_LASER_SPAN_FIELDS]*/,
                                const zh_script_span_table *table, uint32_t flags);                    /* the Trigger loop :149-158 */

/* ---------------------------------------------------------------- detuned voice (examples/example_detuned.zig:31-169)
 * OuterInstrument over Instrument as ONE kernel: a sawtooth whose frequency is warbled by low-passed white noise, enveloped,
 * then low-passed again.  Bit-identical to the reference's stage order; per frame i of a sub-span (Zig lines on the right):
 *   n      = 0 + (rand * 2 - 1)                                                  :139-140  white, one draw per frame
 *   w      = 0 + LP_noise(n; cut = clamp(cutoffFromFrequency(warble_hz, sr)), res 0.0)      :141-150
 *   if ((mode & 1) == 0) w = w * warble_wide                                     :152-154
 *   f      = freq * pow(2.0, w)                   (a store, not an add)          :61-65
 *   o      = 0 + trisaw(t; color);  t += f / sample_rate                         :67-72   TriSawOsc's frequency-buffer path
 *   out1  += f                                    (skipped when outputs[1].ptr is NULL)     :74
 *   o      = o * volume                                                          :76
 *   e      = 0 + env                              (a frame the envelope does not paint keeps the 0)   :78-86
 *   x      = 0 + o * e                            (multiply, round, add: never fused)       :87-88
 *   out0  += LP_main(x; cut = clamp(cutoffFromFrequency(cutoff_hz, sr)), res)    :90-99
 * and after the sub-span t -= trunc(t).  Every `0 +` is zang.zero followed by a module's `+=` (-0.0 becomes +0.0).  Both cutoffs
 * are computed once per sub-span.  note_id_changed reaches the envelope only: the noise, both filters and the oscillator carry
 * their state across notes.  The patch holds the reference's constants; every patch value, sample_rate and freq, hostile ones
 * included, is DEFINED: the voice does what the stage-by-stage composition of the existing paints does with the same value.
 * zh_detuned_create seeds voice v as zh_noise_create does (first_seed + v).  zh_detuned_state.noise.b is not part of the voice
 * (white noise never reads the taps): get_state reports zeros, set_state ignores it; osc.cnt is carried untouched.
 * zh_detuned_paint_spans is the Trigger loop of :213-222 for every voice in one launch, with the contract of
 * zh_laser_paint_spans: empty sub-spans run their prologue, a sub-span out of order ends the voice's list, ZH_PAINT_ZERO_FIRST
 * writes all of [span_start, span_end) of BOTH outputs, ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED; frames outside every sub-span
 * touch no state (the noise does not advance there); a field without a span array takes its value from `params` (a broadcast
 * value or a per-voice device array).  Neither paint allocates or synchronises: both are capturable, and paints, span paints
 * and graph replays of one zh_detuned mix.  outputs[0] = the voice, outputs[1] = the frequency image (the reference's
 * oscilloscope sync); an outputs[1] whose ptr is NULL is not painted.
 * ZH_ERR_INVALID: what zh_laser_paint[_spans] refuses, an outputs[0] that is NULL or too small, an outputs[1] that is not NULL
 * and too small or shares a float with outputs[0] (as zh_stereo_echoes_paint: column ranges of one allocation with one stride do not). */
typedef struct zh_detuned zh_detuned;
typedef struct zh_detuned_patch {          /* the reference's constants; uniform over a call */
    float warble_hz, warble_wide;          /* 4.0, 4.0       :146, :153 */
    float color, volume;                   /* 0.0, 0.75      :71, :76   */
    float attack, decay, release, sustain_volume;   /* cubed 0.025, 0.1, 1.0; 0.5   :81-84 */
    float cutoff_hz, res;                  /* 880.0, 0.8     :95, :98   */
} zh_detuned_patch;
typedef struct zh_detuned_params {                                                                     /* :106-111 */
    float sample_rate; uint32_t reserved;
    zh_f32 freq; zh_bool note_on; zh_u32 mode;     /* broadcast or per-voice device arrays; mode bit 0 set = narrow warble */
    zh_detuned_patch patch;
} zh_detuned_params;
typedef struct zh_detuned_state { zh_noise_state noise; zh_filter_state noise_filter; zh_trisawosc_state osc;
                                  zh_envelope_state env; zh_filter_state main_filter; } zh_detuned_state;   /* :113-115, :41-43 */
enum { ZH_DETUNED_SPAN_FREQ = 0 /* f */, ZH_DETUNED_SPAN_NOTE_ON /* u */, ZH_DETUNED_SPAN_MODE /* u */, ZH_DETUNED_SPAN_FIELDS };
ZH_API int zh_detuned_patch_default(zh_detuned_patch *patch);
ZH_API int zh_detuned_create(zh_ctx *ctx, uint32_t n_voices, uint64_t first_seed, zh_detuned **out);   /* init() :117-123 */
ZH_API int zh_detuned_destroy(zh_detuned *m);
ZH_API int zh_detuned_get_state(zh_detuned *m, zh_detuned_state *host);
ZH_API int zh_detuned_set_state(zh_detuned *m, const zh_detuned_state *host);
ZH_API int zh_detuned_paint(zh_detuned *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                            const zh_buf *temps /*[4], unused; may be NULL*/,
                            zh_bool note_id_changed, const zh_detuned_params *params, uint32_t flags); /* :125-168 */
ZH_API int zh_detuned_paint_spans(zh_detuned *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/, const zh_buf *temps,
                                  const zh_detuned_params *params, const zh_script_span_param *span_params /*[ZH_DETUNED_SPAN_FIELDS]*/,
                                  const zh_script_span_table *table, uint32_t flags);                  /* the Trigger loop :213-222 */

/* ---------------------------------------------------------------- curve voice (examples/example_curve.zig:18-96)
 * CurvePlayer as ONE kernel: two Curves (modulator frequency, carrier frequency) drive a phase-modulated pair of SineOscs.  There
 * is no volume curve: the carrier adds straight into outputs[0], and its frequency image is added into outputs[1] (the reference's
 * oscilloscope sync).  Bit-identical to the reference's stage order; per frame i of a sub-span [s, e), r = i - s (Cm, Cc = the
 * effect's modulator and carrier curves; Zig lines on the right):
 *   f_m    = (0 + Cm(r)) * rel_freq                     (a frame the curve does not paint is +0.0)                 :65-71
 *   p      = 0 + sin((t_m + 0) * pi * 2);  t_m += f_m * (1 / sample_rate)                                          :73-78
 *   f_c    = (0 + Cc(r)) * rel_freq                                                                                :80-86
 *   out0  += sin((t_c + p) * pi * 2);      t_c += f_c * (1 / sample_rate)      (no `0 +`: added into the output itself)   :88-92
 *   out1  += f_c                           (on EVERY frame of the sub-span, a +-0.0 or NaN addend too; skipped when outputs[1].ptr is NULL)   :94
 * and after the sub-span t_m -= trunc(t_m), t_c -= trunc(t_c).  Every `0 +` is zang.zero followed by a module's `+=` (-0.0 becomes
 * +0.0); where the reference zeroes no temp there is none: a sine of -0.0 added to a -0.0 in outputs[0] stays -0.0.
 * The curves come from an effect kit (zh_sfx_kit, above, unchanged): the voice plays effect e's `modulator` and `carrier` and never
 * reads `volume`, which may have count 0.  zh_sfx_effect_curve_example fills in the reference's pair (nodes[0..2] = the modulator
 * of :27-31, nodes[3..8] = the carrier of :18-25, both smoothstep, volume {NULL, 0, smoothstep}).  All of zh_laser's kit semantics
 * carry over: each of the two curves behaves exactly as zh_curve_module_paint does and reads its carried node at the index the
 * previous paint left, counted from the first node of the curve it plays NOW (the kit's zero tail keeps that read inside the
 * array; an index past the array, which only zh_curve_player_set_state can produce, drops the carried node).  An effect index >=
 * the kit's count is DEFINED: nothing is painted, none of the ten state words changes, no node is read and neither output is
 * touched -- even when note_id_changed is set.  A sound outlives buffers (the example's curves run 3.9 s): the state carries it.
 * zh_curve_player_paint_spans is the Trigger loop of :126-129 for every voice in one launch, with the contract of
 * zh_detuned_paint_spans: empty sub-spans run their prologue, a sub-span out of order ends the voice's list, ZH_PAINT_ZERO_FIRST
 * writes all of [span_start, span_end) of BOTH painted outputs (a zero followed by an add paint), ZH_PAINT_TOLERANT is
 * ZH_ERR_UNSUPPORTED; frames outside every sub-span touch nothing; a field without a span array takes its value from `params` (a
 * broadcast value or a per-voice device array).  zh_curve_player_paint is the same kernel over one sub-span per voice.  Neither
 * paint allocates or synchronises: both are capturable, and paints, span paints and graph replays of one zh_curve_player mix.
 * ZH_ERR_INVALID: what zh_laser_paint[_spans] refuses, an outputs[1] that is not NULL and too small or shares a float with outputs[0] (as zh_stereo_echoes_paint: column ranges of one allocation with one stride do not). */
typedef struct zh_curve_player zh_curve_player;
typedef struct zh_curve_player_params {                                                                /* :36-39 */
    float sample_rate; uint32_t reserved;
    zh_f32 rel_freq;
    zh_u32 effect;         /* index into the kit */
    const zh_sfx_kit *kit;
} zh_curve_player_params;
typedef struct zh_curve_player_state {                                                                 /* :41-44 */
    zh_curve_module_state carrier_curve; zh_sineosc_state carrier;
    zh_curve_module_state modulator_curve; zh_sineosc_state modulator;
} zh_curve_player_state;
enum { ZH_CURVE_PLAYER_SPAN_REL_FREQ = 0 /* f */, ZH_CURVE_PLAYER_SPAN_EFFECT /* u */, ZH_CURVE_PLAYER_SPAN_FIELDS };
ZH_API int zh_sfx_effect_curve_example(zh_sfx_effect *effect, zh_curve_node *nodes /*[9]: what the effect's curves point at*/);
ZH_API int zh_curve_player_create(zh_ctx *ctx, uint32_t n_voices, zh_curve_player **out);              /* init() :46-53 */
ZH_API int zh_curve_player_destroy(zh_curve_player *m);
ZH_API int zh_curve_player_get_state(zh_curve_player *m, zh_curve_player_state *host);
ZH_API int zh_curve_player_set_state(zh_curve_player *m, const zh_curve_player_state *host);
ZH_API int zh_curve_player_paint(zh_curve_player *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                                 const zh_buf *temps /*[2], unused; may be NULL*/,
                                 zh_bool note_id_changed, const zh_curve_player_params *params, uint32_t flags);   /* :55-95 */
ZH_API int zh_curve_player_paint_spans(zh_curve_player *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/, const zh_buf *temps,
                                       const zh_curve_player_params *params, const zh_script_span_param *span_params /*[ZH_CURVE_PLAYER_SPAN_FIELDS]*/,
                                       const zh_script_span_table *table, uint32_t flags);             /* the Trigger loop :126-129 */

/* ---------------------------------------------------------------- the monophonic leads: glide and vibrato voices
 * The two lead instruments of the reference's examples, each as ONE kernel.  They share one Params record (sample_rate, freq,
 * note_on) and both paint two outputs: outputs[0] = the voice, outputs[1] = the frequency image (the reference's oscilloscope
 * sync); an outputs[1] whose ptr is NULL is not painted.  Bit-identical to the reference's stage order; every `0 +` below is
 * zang.zero followed by a module's `+=` (-0.0 becomes +0.0), and no multiply is contracted with an add.
 *
 * zh_porta: examples/example_portamento.zig Instrument :20-87.  A sub-span with note_id_changed, freq and note_on begins with
 *   porta.begin(sample_rate, glide_curve, glide, goal = freq, note_on, prev_note_on, note_id_changed)    :55-61
 *   env.begin(note_id_changed = !prev_note_on && note_on), cubed attack / decay / release, sustain_volume :65-73
 *   osc.begin(sample_rate)                          SineOsc's frequency-buffer path, phase constant 0.0  :76-80
 * then per frame i (Zig lines on the right):
 *   g      = 0 + porta                              the glide toward freq, or freq itself once arrived   :53-61
 *   e      = 0 + env                                (a frame the envelope does not paint keeps the 0)    :63-73
 *   s      = 0 + sin((t + 0.0) * 2 pi);  t += g / sample_rate                                            :75-80
 *   out0  += e * s                                  (multiply, round, add: never fused)                  :82
 *   out1  += g                                      (skipped when outputs[1].ptr is NULL)                :85
 * and after the sub-span t -= trunc(t), then prev_note_on = note_on (the `defer` of :51; an empty sub-span runs it too).
 * prev_note_on is the note-level bit the voice carries across sub-spans and buffers: the glide is instantaneous unless
 * note_on && prev_note_on, and the envelope restarts only when every key was up.  The Trigger's note_id_changed reaches the
 * portamento alone (:55).
 *
 * zh_vibrato: examples/example_vibrato.zig Instrument :17-69.  A sub-span begins with vib.begin(sample_rate, vib_hz) and
 * osc.begin(sample_rate, color); per frame i:
 *   m      = 0 + sin((tv + 0.0) * 2 pi);  tv += vib_hz / sample_rate                                     :46-51
 *   f      = freq * (1.0 + depth * m)               (three roundings; a store, not an add)               :52-55
 *   out1  += f                                      (skipped when outputs[1].ptr is NULL)                :56
 *   o      = 0 + pulse(cnt; f, color)               PulseOsc's frequency-buffer path: an f below 0 or above sample_rate / 8
 *                                                   paints nothing, o stays 0 and cnt does not move      :57-62
 *   k      = 0 + (note_on ? 1.0 : nothing)          Gate                                                 :63-66
 *   out0  += o * k                                                                                       :67
 * and after the sub-span tv -= trunc(tv).  note_id_changed reaches no module of this voice: the interface takes it and ignores it.
 *
 * For both: inside a sub-span EVERY frame of out0 and out1 is added to, also when the addend is +-0.0 (a -0.0 already in the image
 * becomes +0.0) and when the PulseOsc paints nothing; frames outside every sub-span touch neither image nor state.  The patches
 * hold the reference's constants; every patch value, sample_rate and freq, hostile ones included, is DEFINED: the voice does what
 * the stage-by-stage composition of the existing paints does with the same value.  zh_X_create starts every voice as init() does
 * (all words zero).
 * zh_X_paint_spans is the Trigger loop (portamento :119-128, vibrato :101-110) for every voice in one launch, with the contract of
 * zh_detuned_paint_spans: empty sub-spans run their prologue and epilogue, a sub-span out of order ends the voice's list,
 * ZH_PAINT_ZERO_FIRST writes all of [span_start, span_end) of BOTH outputs, ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED; a field
 * without a span array takes its value from `params` (a broadcast value or a per-voice device array).  Neither paint allocates
 * or synchronises: both are capturable, and paints, span paints and graph replays of one object mix.
 * ZH_ERR_INVALID: what zh_detuned_paint[_spans] refuses, an outputs[0] that is NULL or too small, an outputs[1] that is not NULL
 * and too small or shares a float with outputs[0] (as zh_stereo_echoes_paint: column ranges of one allocation with one stride do not). */
typedef struct zh_porta zh_porta;
typedef struct zh_porta_patch {            /* the reference's constants; uniform over a call */
    uint32_t glide_curve;                  /* ZH_CURVE_*; ZH_CURVE_CUBED   :57 */
    float glide;                           /* 0.5                          :57 */
    float attack, decay, release, sustain_volume;   /* cubed 0.025, 0.1, 1.0; 0.5   :68-71 */
} zh_porta_patch;
typedef struct zh_porta_params {                                                                       /* :23-27 */
    float sample_rate; uint32_t reserved;
    zh_f32 freq; zh_bool note_on;          /* broadcast or per-voice device arrays */
    zh_porta_patch patch;
} zh_porta_params;
typedef struct zh_porta_state { zh_portamento_state porta; zh_envelope_state env; zh_sineosc_state osc;
                                uint32_t prev_note_on; } zh_porta_state;                               /* :29-32 */
enum { ZH_PORTA_SPAN_FREQ = 0 /* f */, ZH_PORTA_SPAN_NOTE_ON /* u */, ZH_PORTA_SPAN_FIELDS };
ZH_API int zh_porta_patch_default(zh_porta_patch *patch);
ZH_API int zh_porta_create(zh_ctx *ctx, uint32_t n_voices, zh_porta **out);                            /* init() :34-41 */
ZH_API int zh_porta_destroy(zh_porta *m);
ZH_API int zh_porta_get_state(zh_porta *m, zh_porta_state *host);
ZH_API int zh_porta_set_state(zh_porta *m, const zh_porta_state *host);
ZH_API int zh_porta_paint(zh_porta *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                          const zh_buf *temps /*[3], unused; may be NULL*/,
                          zh_bool note_id_changed, const zh_porta_params *params, uint32_t flags);     /* :43-86 */
ZH_API int zh_porta_paint_spans(zh_porta *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/, const zh_buf *temps,
                                const zh_porta_params *params, const zh_script_span_param *span_params /*[ZH_PORTA_SPAN_FIELDS]*/,
                                const zh_script_span_table *table, uint32_t flags);                    /* the Trigger loop :119-128 */

typedef struct zh_vibrato zh_vibrato;
typedef struct zh_vibrato_patch {          /* the reference's constants; uniform over a call */
    float vib_hz, depth, color;            /* 4.0, 0.02, 0.5   :49, :54, :61 */
} zh_vibrato_patch;
typedef struct zh_vibrato_params {                                                                     /* :20-24 */
    float sample_rate; uint32_t reserved;
    zh_f32 freq; zh_bool note_on;          /* broadcast or per-voice device arrays */
    zh_vibrato_patch patch;
} zh_vibrato_params;
typedef struct zh_vibrato_state { zh_sineosc_state vib; zh_pulseosc_state osc; } zh_vibrato_state;     /* :26-28 (the Gate has no state) */
enum { ZH_VIBRATO_SPAN_FREQ = 0 /* f */, ZH_VIBRATO_SPAN_NOTE_ON /* u */, ZH_VIBRATO_SPAN_FIELDS };
ZH_API int zh_vibrato_patch_default(zh_vibrato_patch *patch);
ZH_API int zh_vibrato_create(zh_ctx *ctx, uint32_t n_voices, zh_vibrato **out);                        /* init() :30-36 */
ZH_API int zh_vibrato_destroy(zh_vibrato *m);
ZH_API int zh_vibrato_get_state(zh_vibrato *m, zh_vibrato_state *host);
ZH_API int zh_vibrato_set_state(zh_vibrato *m, const zh_vibrato_state *host);
ZH_API int zh_vibrato_paint(zh_vibrato *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                            const zh_buf *temps /*[3], unused; may be NULL*/,
                            zh_bool note_id_changed, const zh_vibrato_params *params, uint32_t flags); /* :38-68 */
ZH_API int zh_vibrato_paint_spans(zh_vibrato *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/, const zh_buf *temps,
                                  const zh_vibrato_params *params, const zh_script_span_param *span_params /*[ZH_VIBRATO_SPAN_FIELDS]*/,
                                  const zh_script_span_table *table, uint32_t flags);                  /* the Trigger loop :101-110 */

/* ---------------------------------------------------------------- HardSquareInstrument as ONE fused kernel
 * examples/modules.zig:250-289 (a PulseOsc of color 0.5 times a Gate, the reference's only user of Gate) for n voices, with the
 * frequency image examples/example_arpeggiator.zig:115 adds beside it (outputs[1], may be a zh_buf whose ptr is NULL: not painted).
 * Inside a sub-span EVERY frame of outputs[0] gets `+= osc * gate` -- with the gate at 0 and where the PulseOsc paints nothing
 * (freq < 0 or above sample_rate / 8) too, so -0.0 becomes +0.0 and a non-finite osc shows -- and every frame of outputs[1]
 * `+= freq`.  PulseOsc's per-paint prologue runs at every sub-span.  note_id_changed reaches no module of this voice.  Semantics of
 * the span paint: zh_<module>_paint_spans above; ZH_PAINT_ZERO_FIRST writes all of [span_start, span_end) of BOTH outputs,
 * ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED; no host sync: capturable.  ZH_ERR_INVALID: NULL arguments, end < start, an outputs[0]
 * that is NULL or too small, an outputs[1] that is not NULL and too small or shares a float with outputs[0] (as zh_stereo_echoes_paint: column ranges of one allocation with one stride do not), what
 * zh_<module>_paint_spans refuses. */
typedef struct zh_hard_square zh_hard_square;
typedef struct zh_hard_square_params {                                                                 /* modules.zig:253-257 */
    float sample_rate; uint32_t reserved;
    zh_f32 freq; zh_bool note_on;          /* broadcast or per-voice device arrays */
} zh_hard_square_params;
typedef struct zh_hard_square_state { zh_pulseosc_state osc; } zh_hard_square_state;                   /* :259-260 (the Gate has no state) */
enum { ZH_HARD_SQUARE_SPAN_FREQ = 0 /* f */, ZH_HARD_SQUARE_SPAN_NOTE_ON /* u */, ZH_HARD_SQUARE_SPAN_FIELDS };
ZH_API int zh_hard_square_create(zh_ctx *ctx, uint32_t n_voices, zh_hard_square **out);                /* init() modules.zig:262-267 */
ZH_API int zh_hard_square_destroy(zh_hard_square *m);
ZH_API int zh_hard_square_get_state(zh_hard_square *m, zh_hard_square_state *host);
ZH_API int zh_hard_square_set_state(zh_hard_square *m, const zh_hard_square_state *host);
ZH_API int zh_hard_square_paint(zh_hard_square *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                                const zh_buf *temps /*[2], unused; may be NULL*/, zh_bool note_id_changed,
                                const zh_hard_square_params *params, uint32_t flags);                  /* modules.zig:269-288, arpeggiator :115 */
ZH_API int zh_hard_square_paint_spans(zh_hard_square *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                                      const zh_buf *temps, const zh_hard_square_params *params,
                                      const zh_script_span_param *span_params /*[ZH_HARD_SQUARE_SPAN_FIELDS]*/,
                                      const zh_script_span_table *table, uint32_t flags);              /* the Trigger loop, arpeggiator :106-116 */

/* ---------------------------------------------------------------- the arpeggiator stage: held keys -> impulses, ON THE DEVICE
 * Arpeggiator.paint of examples/example_arpeggiator.zig (:49-117) without its instrument, for n players, one lane each: a stage
 * between a live voice bank and a voice.  INPUT: the sub-span table a live bank of polyphony 1 fills from records
 * {held_lo, held_hi, on = 1} (MainModule.paint's bare Trigger, :153-156; keyEvent :159-167 pushes the whole held-key mask), as
 * `in` + held[2] (the `u` arrays of record words 0 and 1), and the key frequencies given at creation (1 to 64 f32, copied to the
 * device: the caller's a4 * rel_freq).  OUTPUT: the stage's own [span][player] table -- count, start, end, note_id_changed, freq,
 * note_on -- which any *_paint_spans reads in place through zh_arp_script_table / zh_arp_span_param (field 0 = freq as `f`,
 * 1 = note_on as `u`).  zh_arp_schedule enqueues ONE kernel: no sync, no copy, capturable.
 * Per player and per outer sub-span [s, e) that holds a note, in order, exactly Arpeggiator.paint (not at all where the outer
 * table has no sub-span: state untouched, no rows):
 *  - note_duration = trunc(0.03f * sample_rate), the product rounded once in f32 (:56); ZH_ERR_INVALID unless 1 <= it < 2^31.
 *  - while next_frame < out_len (the whole buffer's length, :68): the next held key from last_note + 1, wrapping over n_keys;
 *    found: a note-on at its frequency, last_note = it; none and last_note set: a note-off at last_note's frequency; none and no
 *    last_note: nothing.  Every push draws a fresh id; the inner ImpulseQueue accepts 32 a call, last_note and next_id advance
 *    on a dropped push too.  next_frame += note_duration.
 *  - next_frame -= out_len once per call (:104): a buffer with k outer sub-spans moves the clock k buffers.
 *  - the inner Trigger (:106-107) walks [s, e): an impulse at or above e ends the walk (the carried note plays to e, the impulse
 *    is lost); one below the walk's position is taken at the position (the reference asserts; as zh_trigger_next defines it).
 *    note_id_changed: trigger.zig:96-99.
 * The carried note's sample rate is not kept: the voice takes the call's.  OVERFLOW as on a voice bank: a player's list stops at
 * max_spans, state advances, zh_arp_overflows counts dropped rows.  Capacity: 4 rows at creation, zh_arp_reserve changes it
 * (invalidates views; ZH_ERR_UNSUPPORTED while a capture records).  zh_arp_reset: init() :38-47 -- all zero, next_id = 1,
 * last_note = -1.  ZH_ERR_INVALID: NULL arguments, n_keys outside 1..64, max_spans of 0 or above the capacity, a NULL array in
 * `in` or held, in->max_spans == 0; set_state: a last_note outside -1 .. n_keys - 1. */
typedef struct zh_arp zh_arp;
typedef struct zh_arp_state {
    uint64_t next_frame;                   /* :35 */
    uint64_t next_id;                      /* the IdGenerator's (:32) */
    int32_t last_note;                     /* :36; -1 = null */
    uint32_t has_note;                     /* the inner Trigger's carried note (:34, trigger.zig:41) ... */
    uint64_t note_id;
    float freq; uint32_t note_on;          /* ... and its params */
} zh_arp_state;
enum { ZH_ARP_SPAN_FREQ = 0 /* f */, ZH_ARP_SPAN_NOTE_ON /* u */, ZH_ARP_SPAN_FIELDS };
ZH_API int zh_arp_create(zh_ctx *ctx, uint32_t n_players, const float *key_freqs /* host [n_keys] */, uint32_t n_keys, zh_arp **out);
ZH_API int zh_arp_destroy(zh_arp *arp);
ZH_API int zh_arp_reset(zh_arp *arp);                                                                  /* init() :38-47 */
ZH_API int zh_arp_reserve(zh_arp *arp, uint32_t max_rows);
ZH_API int zh_arp_schedule(zh_arp *arp, float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in,
                           const zh_script_span_param *held /*[2]: held_lo, held_hi*/);                /* :49-107 per outer sub-span */
ZH_API int zh_arp_script_table(const zh_arp *arp, uint32_t max_spans, zh_script_span_table *out);
ZH_API int zh_arp_span_param(const zh_arp *arp, uint32_t field /* ZH_ARP_SPAN_* */, zh_script_span_param *out);
ZH_API int zh_arp_overflows(zh_arp *arp, uint64_t *out);
ZH_API int zh_arp_get_state(zh_arp *arp, zh_arp_state *host /*[n_players]*/);
ZH_API int zh_arp_set_state(zh_arp *arp, const zh_arp_state *host);

/* ---------------------------------------------------------------- the key fan-out stage: one always-running voice per key, ON THE DEVICE
 * Polyphony.paint of examples/example_polyphony.zig (:61-92) without its instruments, for n players of n_keys voices, one lane per
 * VOICE: a stage between a live voice bank and a voice.  INPUT: exactly zh_arp_schedule's -- the sub-span table a live bank of
 * polyphony 1 fills from records {held_lo, held_hi, on = 1} (MainModule.paint's Trigger, :137-145; keyEvent :171-176 pushes the
 * whole held-key mask), as `in` + held[2], and the key frequencies given at creation (1 to 64 f32, copied to the device: the
 * caller's a4 * rel_freq).  OUTPUT: the stage's own table of n_players * n_keys columns, voice v = player * n_keys + key (the group
 * layout of zh_mixdown_groups and zh_decimator_paint_groups; n_players * n_keys <= 2^31) -- count, start, end, note_id_changed,
 * freq, note_on -- read in place through zh_keyfan_span_table (the zh_span_table of zh_nice_paint_spans / zh_pmosc_paint_spans) or
 * through zh_keyfan_script_table / zh_keyfan_span_param (any other *_paint_spans; field 0 = freq as `f`, 1 = note_on as `u`).
 * zh_keyfan_schedule enqueues ONE kernel: no sync, no copy, capturable.
 * Per voice and per outer sub-span [s, e) of its player, in order, with bit = the key's bit of the mask (bits at or above n_keys
 * belong to no voice) -- not at all where the outer table has no sub-span: state untouched, no rows:
 *  - bit != down (:70-77): id = next_id++, down = bit, and the impulse (frame 0, id, {freq = key_freqs[key], note_on = bit}) goes to
 *    the voice's Trigger, which takes it at the walk's position s (frame 0 is below s in every sub-span but a buffer's first: the
 *    reference asserts, trigger.zig:161; taken at the position, as zh_trigger_next defines it).  s < e: the row (s, e, freq, bit,
 *    note_id_changed as trigger.zig:96-99: 1 without a carried note, else id != its id), and the note is the carried one.
 *    s == e (no outer Trigger makes one, a caller's table can): no walk, so no row and the carried note stays; down and next_id have
 *    advanced and the impulse is lost with the consumed queue.
 *  - else, with a carried note and s < e: the row (s, e, its freq, its note_on, 0).  Else nothing.
 * in->count above in->max_spans reads the first in->max_spans rows; a sub-span with end < start or end > out_len ends the
 * player's list.  The carried note's sample rate is not kept: the voice takes the call's.  OVERFLOW as on a voice bank: a voice's
 * list stops at max_spans, state advances, zh_keyfan_overflows counts dropped rows; an outer ImpulseQueue holds 32 impulses, so
 * max_spans >= 34 drops nothing behind a live bank.  Capacity: 4 rows at creation, zh_keyfan_reserve changes it (invalidates views;
 * ZH_ERR_UNSUPPORTED while a capture records).  zh_keyfan_reset: Voice :50-56 -- all zero, next_id = 1.  set_state takes any
 * words (`down` is compared as a word, freq is carried as its bits).  ZH_ERR_INVALID: NULL arguments, n_keys outside 1..64,
 * n_players * n_keys above 2^31, max_spans of 0 or above the capacity, a NULL array in `in` or held, in->max_spans == 0, a field
 * at or above ZH_KEYFAN_SPAN_FIELDS. */
typedef struct zh_keyfan zh_keyfan;
typedef struct zh_keyfan_state {
    uint64_t next_id;                      /* the Voice's IdGenerator (:37) */
    uint32_t down;                         /* :35 */
    uint32_t has_note;                     /* the Voice's Trigger's carried note (:39, trigger.zig:41) ... */
    uint64_t note_id;
    float freq; uint32_t note_on;          /* ... and its params */
} zh_keyfan_state;
enum { ZH_KEYFAN_SPAN_FREQ = 0 /* f */, ZH_KEYFAN_SPAN_NOTE_ON /* u */, ZH_KEYFAN_SPAN_FIELDS };
ZH_API int zh_keyfan_create(zh_ctx *ctx, uint32_t n_players, const float *key_freqs /* host [n_keys] */, uint32_t n_keys, zh_keyfan **out);
ZH_API int zh_keyfan_destroy(zh_keyfan *kf);
ZH_API int zh_keyfan_reset(zh_keyfan *kf);                                                             /* Voice :50-56 */
ZH_API int zh_keyfan_reserve(zh_keyfan *kf, uint32_t max_rows);
ZH_API int zh_keyfan_schedule(zh_keyfan *kf, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in,
                              const zh_script_span_param *held /*[2]: held_lo, held_hi*/);             /* :61-92 per outer sub-span */
ZH_API int zh_keyfan_span_table(const zh_keyfan *kf, uint32_t max_spans, zh_span_table *out);
ZH_API int zh_keyfan_script_table(const zh_keyfan *kf, uint32_t max_spans, zh_script_span_table *out);
ZH_API int zh_keyfan_span_param(const zh_keyfan *kf, uint32_t field /* ZH_KEYFAN_SPAN_* */, zh_script_span_param *out);
ZH_API int zh_keyfan_overflows(zh_keyfan *kf, uint64_t *out);
ZH_API int zh_keyfan_get_state(zh_keyfan *kf, zh_keyfan_state *host /*[n_players * n_keys]*/);
ZH_API int zh_keyfan_set_state(zh_keyfan *kf, const zh_keyfan_state *host);

/* ---------------------------------------------------------------- InnerInstrument of the subsong example as ONE fused kernel
 * examples/example_subsong.zig:24-68 for n voices: a TriSawOsc of constant frequency (temps[0], zeroed first) times an Envelope
 * whose three curves are cubed (temps[1], zeroed first), `outputs[0] += temps[0] * temps[1]` (:66).  Inside a sub-span EVERY
 * frame of outputs[0] gets `+= osc * env` -- where the TriSawOsc paints nothing (freq < 0 or above sample_rate / 8) osc is the
 * zero of :51, where the Envelope paints nothing (idle; note_on while releasing) env is the zero of :57: -0.0 becomes +0.0 and a
 * non-finite factor shows.  Both modules' per-paint prologues run at every sub-span; note_id_changed reaches the Envelope.  The
 * oscillator's f32 phase `t` is state the constant-frequency path never touches.  Semantics of the span paint:
 * zh_<module>_paint_spans above; ZH_PAINT_ZERO_FIRST is supported, ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED; no host sync:
 * capturable.  ZH_ERR_INVALID: NULL arguments, end < start, an outputs[0] that is NULL or too small, what
 * zh_<module>_paint_spans refuses. */
typedef struct zh_saw_env zh_saw_env;
typedef struct zh_saw_env_patch {          /* the reference's constants; uniform over a call */
    float color;                           /* 0.0                                    :55 */
    float attack, decay, release;          /* cubed durations 0.025, 0.1, 0.15       :60-62 */
    float sustain_volume;                  /* 0.5                                    :63 */
} zh_saw_env_patch;
typedef struct zh_saw_env_params {                                                                     /* :27-31 */
    float sample_rate; uint32_t reserved;
    zh_f32 freq; zh_bool note_on;          /* broadcast or per-voice device arrays */
    zh_saw_env_patch patch;
} zh_saw_env_params;
typedef struct zh_saw_env_state { zh_trisawosc_state osc; zh_envelope_state env; } zh_saw_env_state;   /* :33-34 */
enum { ZH_SAW_ENV_SPAN_FREQ = 0 /* f */, ZH_SAW_ENV_SPAN_NOTE_ON /* u */, ZH_SAW_ENV_SPAN_FIELDS };
ZH_API int zh_saw_env_patch_default(zh_saw_env_patch *patch);
ZH_API int zh_saw_env_create(zh_ctx *ctx, uint32_t n_voices, zh_saw_env **out);                        /* init() :36-41 */
ZH_API int zh_saw_env_destroy(zh_saw_env *m);
ZH_API int zh_saw_env_get_state(zh_saw_env *m, zh_saw_env_state *host);
ZH_API int zh_saw_env_set_state(zh_saw_env *m, const zh_saw_env_state *host);
ZH_API int zh_saw_env_paint(zh_saw_env *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[1]*/,
                            const zh_buf *temps /*[2], unused; may be NULL*/, zh_bool note_id_changed,
                            const zh_saw_env_params *params, uint32_t flags);                          /* :43-67 */
ZH_API int zh_saw_env_paint_spans(zh_saw_env *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[1]*/,
                                  const zh_buf *temps, const zh_saw_env_params *params,
                                  const zh_script_span_param *span_params /*[ZH_SAW_ENV_SPAN_FIELDS]*/,
                                  const zh_script_span_table *table, uint32_t flags);                  /* the Trigger loop :135-143 */

/* ---------------------------------------------------------------- melody kits: K canned songs resident on the device
 * A song is what NoteTracker follows (src/zang/notes.zig:130-134, :138-153): events {t seconds, note_id, params {freq, note_on}}
 * in chronological order.  zh_melody_kit_create copies K of them into one device blob -- melody m is events [offsets[m],
 * offsets[m + 1]) of `events` -- immutable afterwards; it synchronises and is not capturable; the caller's arrays may be freed on
 * return.  n_melodies == 0 and empty melodies are legal.  The reference asserts the order (notes.zig:177); here ZH_ERR_INVALID:
 * NULL arguments (events may be NULL when n_events is 0), a t that is NaN or negative, a t below the one before it in the same
 * melody, offsets that decrease, an offset above n_events.  Destroy a kit after every stage that plays it. */
typedef struct zh_melody_kit zh_melody_kit;
typedef struct zh_melody_event {           /* SongEvent, notes.zig:130-134 */
    float t;                               /* seconds from the melody's start */
    uint32_t note_on;
    uint64_t note_id;
    float freq; uint32_t reserved;
} zh_melody_event;
ZH_API int zh_melody_kit_create(zh_ctx *ctx, const uint32_t *offsets /* host [n_melodies + 1] */, uint32_t n_melodies,
                                const zh_melody_event *events /* host [n_events] */, uint32_t n_events, zh_melody_kit **out);
ZH_API int zh_melody_kit_destroy(zh_melody_kit *kit);
ZH_API int zh_melody_kit_count(const zh_melody_kit *kit, uint32_t *melodies_out, uint32_t *events_out /* may be NULL */);

/* ---------------------------------------------------------------- the subsong stage: notes within notes, ON THE DEVICE
 * SubtrackPlayer.paint of examples/example_subsong.zig (:122-144) without its instrument, for n players, one lane each: a stage
 * between a live voice bank and a voice.  INPUT: the sub-span table a live bank of polyphony 1 fills from records
 * {freq, note_on, melody} (MainModule.paint's Trigger, :176-185; keyEvent :188-201), as `in` + outer[3] (ZH_SUBSONG_IN_*: freq as
 * `f`, note_on as `u`, melody as `u`), and a melody kit.  OUTPUT: the stage's own [span][player] table -- count, start, end,
 * note_id_changed, freq, note_on -- which any *_paint_spans reads in place through zh_subsong_script_table /
 * zh_subsong_span_param (field 0 = freq as `f`, 1 = note_on as `u`).  zh_subsong_schedule enqueues ONE kernel: no sync, no copy,
 * capturable.  Per player and per outer sub-span [s, e) with (freq_o, on_o, nic_o), in order, exactly SubtrackPlayer.paint:
 *  - on_o && nic_o (:130-133): next_song_event = 0, t = 0, the inner Trigger forgets its note, and the player's melody is
 *    latched from this sub-span's `melody` (ignored on every other sub-span); an index at or above K latches
 *    UINT32_MAX ("no melody"), an empty song.
 *  - NoteTracker.consume(sample_rate, [s, e)) (notes.zig:162-206) in f32, nothing fused: out_len = e - s (the SUB-SPAN's),
 *    buf_time = out_len / sample_rate, end_t = t + buf_time; every next event with note_t < end_t becomes an impulse at
 *    s + min(trunc(((note_t - t) / buf_time) * out_len), out_len - 1), the conversion NaN -> 0 and saturating; t = end_t.  The
 *    reference's arrays hold 32: a 33rd event of one call advances next_song_event and is dropped.
 *  - the inner Trigger (:135-136; trigger.zig:80-196) walks [s, e) over those impulses; an impulse below the walk's position (a
 *    clock that runs backwards: a negative sample rate) is taken at the position (the reference asserts; as zh_trigger_next).
 *  - one row per inner sub-span: freq = (freq_i * freq_o) / base_freq, two f32 operations in that order (:140), freq_i the
 *    song's RAW frequency and freq_o THIS outer sub-span's -- the carried note keeps the raw value, so a key change re-scales a
 *    held melody note; note_on the song's; note_id_changed = (on_o && nic_o) || the inner Trigger's (:137), which compares the
 *    song's note_id (trigger.zig:96-99): a note-off that shares its note-on's id is not a new note.
 * Defined where the reference is not.  An outer sub-span with e <= s or e > out_len ends the player's list (out_len is an
 * argument for this alone).  OVERFLOW as on a voice bank: a player's list stops at max_spans, state advances,
 * zh_subsong_overflows counts dropped rows.  Capacity: 33 rows at creation (what one outer sub-span can make),
 * zh_subsong_reserve changes it (invalidates views; ZH_ERR_UNSUPPORTED while a capture records).  A sample_rate that is 0,
 * negative, NaN or infinite follows the arithmetic above: nothing is refused for the rate.  zh_subsong_reset: init() :104-120 --
 * all zero, the melody 0 (the reference's one song; UINT32_MAX on an empty kit): an outer note-off with no earlier
 * note-on runs melody 0 from its start without a reset.  The kit must outlive the stage.  ZH_ERR_INVALID: NULL arguments, a kit of
 * another context, a base_freq that is NaN, max_spans of 0 or above the capacity, a NULL array in `in` (note_id_changed
 * included) or outer, in->max_spans == 0; set_state: a melody that is neither below K nor UINT32_MAX. */
typedef struct zh_subsong zh_subsong;
typedef struct zh_subsong_state {
    uint32_t next_song_event;              /* NoteTracker's (notes.zig:140) */
    float t;                               /* notes.zig:141 */
    uint32_t melody;                       /* the latched melody, or UINT32_MAX: none */
    uint32_t has_note;                     /* the inner Trigger's carried note (:102, trigger.zig:41) ... */
    uint64_t note_id;
    float freq; uint32_t note_on;          /* ... and its params: the song's raw freq */
} zh_subsong_state;
enum { ZH_SUBSONG_IN_FREQ = 0 /* f */, ZH_SUBSONG_IN_NOTE_ON /* u */, ZH_SUBSONG_IN_MELODY /* u */, ZH_SUBSONG_IN_FIELDS };
enum { ZH_SUBSONG_SPAN_FREQ = 0 /* f */, ZH_SUBSONG_SPAN_NOTE_ON /* u */, ZH_SUBSONG_SPAN_FIELDS };
ZH_API int zh_subsong_create(zh_ctx *ctx, uint32_t n_players, const zh_melody_kit *kit, float base_freq /* :98 */, zh_subsong **out);
ZH_API int zh_subsong_destroy(zh_subsong *sub);
ZH_API int zh_subsong_reset(zh_subsong *sub);                                                          /* init() :104-120 */
ZH_API int zh_subsong_reserve(zh_subsong *sub, uint32_t max_rows);
ZH_API int zh_subsong_schedule(zh_subsong *sub, float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table *in,
                               const zh_script_span_param *outer /*[ZH_SUBSONG_IN_FIELDS]*/);          /* :122-144 per outer sub-span */
ZH_API int zh_subsong_script_table(const zh_subsong *sub, uint32_t max_spans, zh_script_span_table *out);
ZH_API int zh_subsong_span_param(const zh_subsong *sub, uint32_t field /* ZH_SUBSONG_SPAN_* */, zh_script_span_param *out);
ZH_API int zh_subsong_overflows(zh_subsong *sub, uint64_t *out);
ZH_API int zh_subsong_get_state(zh_subsong *sub, zh_subsong_state *host /*[n_players]*/);
ZH_API int zh_subsong_set_state(zh_subsong *sub, const zh_subsong_state *host);

/* ---------------------------------------------------------------- the merge stage: two span tables into one, ON THE DEVICE
 * The loop of examples/example_two.zig:93-151 ("an iterator that consumes two source iterators") without its voice, for n
 * players, one lane each: one voice driven by two impulse streams.  INPUT: two [span][player] tables A and B (e.g. of two live
 * banks of polyphony 1) with their field arrays, as the source descriptors given at creation name them: n_fields (1..4), the
 * kind of each ('f' or 'u', as zh_script_span_param), and on_field, the index of the source's note-on field (kind 'u').
 * OUTPUT: the stage's own table, which any *_paint_spans reads in place through zh_span_merge_script_table /
 * zh_span_merge_span_param.  Its fields, in order: A's, then B's, each with its declared kind (the words copied as bits), then
 * n_a + n_b + ZH_SPAN_MERGE_NOTE_ON, + ZH_SPAN_MERGE_NIC_A, + ZH_SPAN_MERGE_NIC_B, all `u`.  zh_span_merge_schedule enqueues ONE
 * kernel: no sync, no copy, capturable.  The stage keeps no state between buffers (the Triggers live in the banks).
 * Per player, with span = [0, out_len), cnt_x = min(count_x, in_x->max_spans), ia = ib = 0, pos = 0; while pos < out_len and both
 * sources have a row left:
 *    e = min(end_a[ia], end_b[ib]);  e <= pos or e > out_len ends the player's list (defined where the reference is not)
 *    a row [pos, e) with A's fields of row ia and B's of row ib, nic_a = A's note_id_changed[ia], nic_b = B's [ib],
 *       note_on = on_a | on_b (:136),  note_id_changed = (nic_a & on_a & !nic_b) | (nic_b & on_b & !nic_a) (:127-129)
 *    a source whose row ends at e moves to its next row (:139-144; both on a tie);  pos = e
 * Three consequences of the reference's text, kept: (a) a source's nic STICKS -- it is set on every merged row cut from the same
 * source row (result0 is the same object until trig0.next runs), only the other source's nic masks it; (b) the sources' `start`
 * arrays are never read: a source whose first row begins after frame 0 is merged from frame 0 with that row's values; (c)
 * nothing follows once either source runs out of rows (the break of :150).
 * OVERFLOW as on a voice bank: a player's list stops at max_spans, zh_span_merge_overflows counts dropped rows.  Capacity: 67
 * rows at creation (what two 34-row tables can make), zh_span_merge_reserve changes it (invalidates views; ZH_ERR_UNSUPPORTED
 * while a capture records).  ZH_ERR_INVALID: NULL arguments, a NULL array (start included) or max_spans == 0 in
 * either table, max_spans of 0 or above the capacity, a field array that lacks the pointer of its kind, n_fields outside 1..4, a
 * kind that is neither 'f' nor 'u', an on_field that is out of range or not of kind 'u'. */
typedef struct zh_span_merge zh_span_merge;
enum { ZH_SPAN_MERGE_MAX_FIELDS = 4 };
typedef struct zh_span_merge_source {
    uint32_t n_fields;                     /* 1..ZH_SPAN_MERGE_MAX_FIELDS */
    uint32_t on_field;                     /* the note-on field: < n_fields, of kind 'u' */
    uint8_t kinds[4];                      /* 'f' or 'u' per field */
} zh_span_merge_source;
/* the stage's own fields, counted from n_fields of A + n_fields of B */
enum { ZH_SPAN_MERGE_NOTE_ON = 0 /* u */, ZH_SPAN_MERGE_NIC_A /* u */, ZH_SPAN_MERGE_NIC_B /* u */, ZH_SPAN_MERGE_OWN_FIELDS };
ZH_API int zh_span_merge_create(zh_ctx *ctx, uint32_t n_players, const zh_span_merge_source *a, const zh_span_merge_source *b,
                                zh_span_merge **out);
ZH_API int zh_span_merge_destroy(zh_span_merge *m);
ZH_API int zh_span_merge_reserve(zh_span_merge *m, uint32_t max_rows);
ZH_API int zh_span_merge_schedule(zh_span_merge *m, uint32_t out_len, uint32_t max_spans,
                                  const zh_script_span_table *in_a, const zh_script_span_param *fields_a /*[a.n_fields]*/,
                                  const zh_script_span_table *in_b, const zh_script_span_param *fields_b /*[b.n_fields]*/);   /* :93-151 */
ZH_API int zh_span_merge_script_table(const zh_span_merge *m, uint32_t max_spans, zh_script_span_table *out);
ZH_API int zh_span_merge_span_param(const zh_span_merge *m, uint32_t field, zh_script_span_param *out);
ZH_API int zh_span_merge_overflows(zh_span_merge *m, uint64_t *out);

/* ---------------------------------------------------------------- the two-source TriSaw voice as ONE fused kernel
 * What one inner span of examples/example_two.zig:109-138 and the multiply of :153 do, for n voices: a TriSawOsc of constant
 * freq and color with note_id_changed false (temps[0], zeroed first) times an Envelope whose three curves are cubed (temps[1],
 * zeroed first; it takes the sub-span's note_id_changed), `outputs[0] += temps[0] * temps[1]` on EVERY frame of the sub-span (the
 * product is rounded, then added; where the TriSawOsc paints nothing -- freq < 0 or above sample_rate / 8 -- or the Envelope
 * paints nothing, the factor is the zero: -0.0 becomes +0.0 and a non-finite factor shows), and `outputs[1] += freq` (:109, the
 * oscilloscope sync; outputs[1] may be a zh_buf whose ptr is NULL: not painted).  Both modules' per-paint prologues run at every
 * sub-span.  ONE DIFFERENCE from the example: it multiplies over the whole buffer (:153), so frames no inner span covers get
 * `+= 0 * 0` there and a -0.0 already in the output becomes +0.0; the span-paint contract leaves such frames alone.  With
 * ZH_PAINT_ZERO_FIRST, which the player uses, the two are identical.  Semantics of the span paint: zh_<module>_paint_spans above;
 * ZH_PAINT_ZERO_FIRST writes all of [span_start, span_end) of BOTH outputs, ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED; no host sync:
 * capturable.  ZH_ERR_INVALID: NULL arguments, end < start, an outputs[0] that is NULL or too small, an outputs[1] that is not
 * NULL and too small or shares a float with outputs[0] (as zh_stereo_echoes_paint: column ranges of one allocation with one stride do not), what
 * zh_<module>_paint_spans refuses. */
typedef struct zh_dual zh_dual;
typedef struct zh_dual_patch {             /* the reference's constants; uniform over a call */
    float attack, decay, release;          /* cubed durations 0.025, 0.1, 1.0        :132-134 */
    float sustain_volume;                  /* 0.5                                    :135 */
} zh_dual_patch;
typedef struct zh_dual_params {
    float sample_rate; uint32_t reserved;
    zh_f32 freq, color; zh_bool note_on;   /* broadcast or per-voice device arrays */
    zh_dual_patch patch;
} zh_dual_params;
typedef struct zh_dual_state { zh_trisawosc_state osc; zh_envelope_state env; } zh_dual_state;         /* :36-37 */
enum { ZH_DUAL_SPAN_FREQ = 0 /* f */, ZH_DUAL_SPAN_COLOR /* f */, ZH_DUAL_SPAN_NOTE_ON /* u */, ZH_DUAL_SPAN_FIELDS };
ZH_API int zh_dual_patch_default(zh_dual_patch *patch);
ZH_API int zh_dual_create(zh_ctx *ctx, uint32_t n_voices, zh_dual **out);                              /* init() :52-53 */
ZH_API int zh_dual_destroy(zh_dual *m);
ZH_API int zh_dual_get_state(zh_dual *m, zh_dual_state *host);
ZH_API int zh_dual_set_state(zh_dual *m, const zh_dual_state *host);
ZH_API int zh_dual_paint(zh_dual *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                         const zh_buf *temps /*[2], unused; may be NULL*/, zh_bool note_id_changed,
                         const zh_dual_params *params, uint32_t flags);                                /* :109-138, :153 */
ZH_API int zh_dual_paint_spans(zh_dual *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[2]*/,
                               const zh_buf *temps, const zh_dual_params *params,
                               const zh_script_span_param *span_params /*[ZH_DUAL_SPAN_FIELDS]*/,
                               const zh_script_span_table *table, uint32_t flags);                     /* the merge loop :101-151 */

/* ---------------------------------------------------------------- the controlled phase-modulation voice as ONE fused kernel
 * The PMOscInstrument of examples/example_mouse.zig:24-73 for n voices, one lane each: the PhaseModOscillator of
 * examples/modules.zig:6-77 times an Envelope whose three curves are cubed.  Against zh_pmosc_* (modules.zig:80-128) `relative`
 * is a parameter, ratio and multiplier are zang.ConstantOrBuffer SIGNALS and the release is a patch constant.  Per frame inside
 * a note sub-span, with r = the ratio and m = the multiplier at the frame (every `0 +` is a zang.zero followed by a module's
 * `+=`; no product is contracted with an add; s: "ONE DIFFERENCE" below):
 *    mf   = relative ? s + r * freq : r       ratio a buffer, modules.zig:50-56 (multiplyScalar is `+=`; copy is a store)
 *           relative ? freq * r     : r       ratio a constant, :43-49 (zang.set: s is not read)
 *    mo   = 0 + sin((tm + 0.0) * 2 pi);  tm += mf * (1 / sample_rate)        the modulator, SineOsc's frequency-buffer path  :58-63
 *    ph   = 0 + mo * m                                                       :64-68
 *    c    = 0 + sin((tc + ph) * 2 pi);   tc += freq / sample_rate            the carrier, as zh_pmosc has it                 :69-74
 *    o    = 0 + c                                                            :75 into the instrument's zeroed temps[0]
 *    e    = 0 + env        (a frame the Envelope does not paint keeps the 0)                          example_mouse.zig:62-70
 *    out += o * e                                                            :71 (the product is rounded, then added)
 * Both oscillators' epilogues (t -= trunc(t)) run at the end of every sub-span, both prologues and the Envelope's at the start of
 * each; note_id_changed goes to all three modules.  Frames outside every note sub-span touch neither the output nor the voice's
 * state.
 * ONE DIFFERENCE, made explicit: the reference's oscillator adds `r * freq` into ITS temps[0] without zeroing it first
 * (modules.zig:52), and that row is the instrument's temps[1], into which the instrument later paints the Envelope
 * (example_mouse.zig:62-63): s at frame i is the envelope value of the last paint that covered buffer index i.  Here the paints
 * take temps[3]: if temps is not NULL and temps[1].ptr is not NULL, that [frame][voice] image is read as s before the frame (in
 * the relative / buffer branch only) and e is stored into it after the frame (in every branch); the caller keeps the image between
 * calls, and that is the reference bit for bit.  If it is NULL, s = +0.0 and nothing is stored.  temps[0] and temps[2] are never
 * touched.
 * zh_pmctl_paint is `paint` of :46-72: a constant ratio / multiplier may be per-voice, a buffer is a [frame][voice] image indexed
 * by ABSOLUTE frame.  zh_pmctl_paint_spans is the Trigger loop of :193-211 over a table of notes with the contract of
 * zh_porta_paint_spans.  zh_pmctl_paint_controlled is the whole of MainModule.paint (:148-211) in one kernel: each control is the
 * Trigger loop of :151-169 / :175-190 around a Portamento -- at each of ITS sub-spans porta.begin(sample_rate, patch.ctl_curve,
 * patch.ctl_glide, goal = value * scale, note_on, prev_note_on = true, that sub-span's note_id_changed); at a frame inside one of
 * its sub-spans the control's value is 0 + the Portamento's frame, outside all of them +0.0 (:149, :172) and its state does not
 * move.  The three streams' boundaries are unrelated; each table follows the contract of zh_detuned_paint_spans on its own (an
 * empty sub-span runs its prologue and epilogue; a sub-span out of order ends THAT stream's list while the other two go on);
 * the controls advance over all of [span_start, span_end) whether or not a note sounds.  In this form the ratio and the
 * multiplier are buffers (the relative / buffer branch reads s).
 * The three paints allocate nothing and never synchronise: capturable.  ZH_PAINT_ZERO_FIRST writes all of [span_start, span_end)
 * of outputs[0]; ZH_PAINT_TOLERANT is ZH_ERR_UNSUPPORTED.  ZH_ERR_INVALID: what zh_dual_paint[_spans] refuses, a zh_cob with an
 * unknown tag, a cob buffer or a temps[1] that is too small, a control that is NULL or has a NULL table, table array, value.f or
 * note_on.u, a value with `u` or a note_on with `f`. */
typedef struct zh_pmctl zh_pmctl;
typedef struct zh_pmctl_patch {            /* the reference's constants; uniform over a call */
    uint32_t ctl_curve; float ctl_glide;   /* ZH_CURVE_LINEAR, 0.1        example_mouse.zig:160, :184 */
    float attack, decay, release, sustain_volume;   /* cubed 0.025, 0.1, 1.0; 0.5   :65-68 */
} zh_pmctl_patch;
typedef struct zh_pmctl_params {
    float sample_rate; uint32_t reserved;
    zh_f32 freq; zh_bool note_on; zh_bool relative;   /* broadcast or per-voice device arrays */
    zh_pmctl_patch patch;
} zh_pmctl_params;
typedef struct zh_pmctl_state { zh_portamento_state ratio, multiplier; zh_sineosc_state carrier, modulator; zh_envelope_state env; } zh_pmctl_state;
enum { ZH_PMCTL_SPAN_FREQ = 0 /* f */, ZH_PMCTL_SPAN_NOTE_ON /* u */, ZH_PMCTL_SPAN_FIELDS };
typedef struct zh_pmctl_control {
    const zh_script_span_table *table;     /* the control's own sub-spans, e.g. of a live bank of polyphony 1 */
    zh_script_span_param value;            /* f: result.params.value */
    zh_script_span_param note_on;          /* u: result.params.note_on */
    zh_f32 scale;                          /* goal = value * scale: 4.0 or 880.0 (:161-164), 2.0 (:185); one f32 multiply */
} zh_pmctl_control;
ZH_API int zh_pmctl_patch_default(zh_pmctl_patch *patch);
ZH_API int zh_pmctl_create(zh_ctx *ctx, uint32_t n_voices, zh_pmctl **out);                            /* init(): every word zero */
ZH_API int zh_pmctl_destroy(zh_pmctl *m);
ZH_API int zh_pmctl_get_state(zh_pmctl *m, zh_pmctl_state *host);
ZH_API int zh_pmctl_set_state(zh_pmctl *m, const zh_pmctl_state *host);
ZH_API int zh_pmctl_paint(zh_pmctl *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[1]*/,
                          const zh_buf *temps /*[3]; NULL or temps[1].ptr NULL: no carried image*/, zh_bool note_id_changed,
                          const zh_pmctl_params *params, const zh_cob *ratio, const zh_cob *multiplier, uint32_t flags);   /* :46-72 */
ZH_API int zh_pmctl_paint_spans(zh_pmctl *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[1]*/,
                                const zh_buf *temps /*[3]*/, const zh_pmctl_params *params,
                                const zh_script_span_param *span_params /*[ZH_PMCTL_SPAN_FIELDS]*/,
                                const zh_script_span_table *table, const zh_cob *ratio, const zh_cob *multiplier,
                                uint32_t flags);                                                       /* the Trigger loop :193-211 */
ZH_API int zh_pmctl_paint_controlled(zh_pmctl *m, uint32_t span_start, uint32_t span_end, const zh_buf *outputs /*[1]*/,
                                     const zh_buf *temps /*[3]*/, const zh_pmctl_params *params,
                                     const zh_script_span_param *span_params /*[ZH_PMCTL_SPAN_FIELDS]*/,
                                     const zh_script_span_table *notes_table, const zh_pmctl_control *ratio_ctl,
                                     const zh_pmctl_control *multiplier_ctl, uint32_t flags);          /* MainModule.paint :148-211 */

/* The zangscript compiler itself (host side, no GPU work): src/zangscript/{tokenize,parse,codegen}.zig restated in
 * C++ (csrc/zscript_front.hip) with both backends (csrc/zscript_emit.hip): the reference's Zig text
 * (codegen_zig.zig; pins the front-end against the golden of src/zangscript/tests.zig:44-92) and the HIP source
 * zh_script_load takes.  `packages`: bit 0 = zang_builtin_package, bit 1 = modules_builtin_package
 * (builtins.zig:153-185).  A compile error returns ZH_ERR_INVALID with the message fail() would print
 * (`file:line:col: message`, source line, carets) in `err`.  Texts are malloc'ed: zh_zscript_free_text. */
typedef struct zh_zscript zh_zscript;
ZH_API int zh_zscript_compile(const char *text, const char *filename, uint32_t packages, zh_zscript **out, char *err, size_t err_cap);
ZH_API int zh_zscript_destroy(zh_zscript *z);
ZH_API void zh_zscript_free_text(char *text);
ZH_API int zh_zscript_generate_zig(zh_zscript *z, char **text_out);
/* only_csv: comma-separated exported module names, NULL = all; unroll: frames per unrolled chunk, 0 = automatic */
ZH_API int zh_zscript_generate_hip(zh_zscript *z, const char *only_csv, int unroll, char **text_out);
/* The same with more kernel forms per module.  ZH_ZSCRIPT_FORM_ROLES: next to zs_paint_<name> (one wave per 64 voices, the
 * whole frame body in every lane) a zs_paint_pc_<name> for FEW voices -- one workgroup of several waves per 64 voices, the
 * body's builtin calls (codegen.zig:70-121: the instruction list being scheduled) dealt to producer / recurrence / writer
 * waves that hand values on through LDS tiles, as the hand-written composites do (examples/modules.zig:130-187 is the
 * acceptance recipe).  Same operations on the same values in the same order: same bits.  zh_script_module_paint picks
 * the form (dispatch table rows script_pc / script_pc_maxv). */
/* ZH_ZSCRIPT_FORM_ROLES: for every module that has more than one role.  ZH_ZSCRIPT_FORM_ROLES_WORTH: only where the emitter's
 * estimate says it pays (a chain that can not be cut into frame ranges, the longest role well below the whole body): about half
 * the hiprtc time of the former (profiles/r06/script_compile_times.txt). */
#define ZH_ZSCRIPT_FORM_ROLES 1
#define ZH_ZSCRIPT_FORM_ROLES_WORTH 2
ZH_API int zh_zscript_generate_hip_forms(zh_zscript *z, const char *only_csv, int unroll, uint32_t forms, char **text_out);
/* per module of the last zh_zscript_generate_hip: what zh_script_module_create / _paint need */
ZH_API uint32_t zh_zscript_module_count(zh_zscript *z);
ZH_API int zh_zscript_module_info(zh_zscript *z, uint32_t i, char *name, size_t name_cap, uint32_t *state_words, uint32_t *noise_fields,
                                  uint32_t *n_params, char *error /* non-empty: the HIP backend cannot express this module */, size_t error_cap);
/* `pub const num_temps` of the generated Zig struct (codegen_zig.zig:518): what a reference host would allocate for this
 * module; the fused kernel itself needs none. */
ZH_API int zh_zscript_module_num_temps(zh_zscript *z, uint32_t i, uint32_t *num_temps);
ZH_API int zh_zscript_module_param(zh_zscript *z, uint32_t i, uint32_t p, char *name, size_t name_cap, char *kind, size_t kind_cap,
                                   char *enum_name, size_t enum_cap);

/* ---------------------------------------------------------------- spectrum analyser (examples/common/fft.zig, examples/visual.zig)
 * What the example harness does with every MainModule's output_visualize buffer, 1,024 frames at a time, for every voice of a
 * [frame][voice] image in ONE kernel (csrc/spectrum.hip): the radix-2 FFT of fft.zig:3-60 on a workgroup's tile in LDS, then one of
 * three epilogues.  Bit-identical to the reference, whose transform has three quirks that are kept:
 *   - twiddles by recurrence: u_1, u_2 are rotated by (c, s) in f32 and (c, s) halved by sqrt per stage (:36-58); they are up to
 *     3.6e-4 from exp(-2 pi i j / n) and the result about 3e-4 of max|X| from an exact FFT's.  No other FFT is bit-comparable.
 *   - the three-multiply butterfly t2 = (re - im) * u_2; t1 = t2 + re * (u_1 - u_2); t2 = t2 + im * (u_1 + u_2) (:45-51), each
 *     statement rounded in f32, nothing fused.
 *   - both widgets read fft_real ONLY (visual.zig:269, :430): a sine exactly on bin 100 shows next to nothing at bin 100 (its energy
 *     is in fft_imag), a cosine 0.7071069.
 * DEFINED where the reference is not: a float-to-u32 cast saturates and NaN casts to 0 (the channel bytes of hslToRgb, the bin index
 * of getFFTValue); height < 2 is refused (the reference divides by height - 1); n must be a power of two >= 2 (fftBitReverse
 * underflows at 1).
 * The twiddle pairs live in a table of the context, built and uploaded by the FIRST of these calls on it (that one call allocates
 * and synchronises; inside a capture it returns ZH_ERR_UNSUPPORTED instead).  No later call allocates, copies or synchronises:
 * all may be recorded into a graph.  Dispatch rows spectrum_tile / spectrum_stages pick the tile width and the schedule (same bits).
 * ZH_ERR_INVALID: NULL arguments, n not a power of two in [2, 1024], rows outside an image, images of different voice counts or
 * that overlap, out.frames < 512, height < 2, row_stride_pixels < voices.  Zero voices: ZH_OK, nothing launched. */
/* fft.zig:26-58, host only, no device: the n - 1 pairs (u_1, u_2) the loops walk through, u[2 k] = u_1 and u[2 k + 1] = u_2; stage
 * l1 = 1, 2, 4, ... contributes l1 pairs, in stage order, so the table of a smaller n is a prefix (1,023 pairs = 8 KiB at 1,024). */
ZH_API int zh_fft_twiddles(float *u /*[2 * (n - 1)]*/, uint32_t n);
/* fft(N, re, im) (:25-60) for every voice, in place on rows [frame_start, frame_start + n) of both images */
ZH_API int zh_fft(zh_ctx *ctx, uint32_t n, uint32_t frame_start, zh_buf re, zh_buf im);
/* DrawSpectrum.plot (visual.zig:257-280) on rows [frame_start, frame_start + 1024) of `samples`: out[k][v] = sqrt(|fft_real[k]| *
 * (1 / 1024)) for k in [0, 512) -- assigned, not added; rows from 512 on are not touched.  `samples` is read once; there is no
 * imaginary image and no scratch. */
ZH_API int zh_spectrum_plot(zh_ctx *ctx, uint32_t frame_start, zh_buf samples, zh_buf out);
/* The column DrawSpectrumFull.plot (visual.zig:411-452) draws: pixel i in [0, height) of voice v -- getFFTValue(i / (height - 1))
 * (:141-159: position f * 511.5, or ((pow(10, f) - 1) / 9) * 511.5 when `logarithmic`; the blend of bins floor and min(511, floor +
 * 1)) of fft_real, coloured hslToRgb(sqrt(|value| / 1024), 1, 0.5) (:88-125; 0xFF000000 | b << 16 | g << 8 | r, the bytes
 * overlapping where the value exceeds 1,024) or 0xFFFF0000 for a NaN -- goes to pixels[(height - 1 - i) * row_stride_pixels + v],
 * `pixels` a device pointer.  A spectrogram buffer is [height][width][voice]: pass pixels + drawindex * voices and row_stride_pixels =
 * width * voices; the stores stay voice-contiguous. */
ZH_API int zh_spectrum_column(zh_ctx *ctx, uint32_t frame_start, zh_buf samples, uint32_t *pixels, size_t row_stride_pixels,
                              uint32_t height, int logarithmic);

/* ---------------------------------------------------------------- event scheduling (host side; no GPU work)
 * The immediate caller of every paint: song / key events -> impulses ->
 * per-voice (span, params, note_id_changed) tuples.  A C++ restatement of src/zang/notes.zig and
 * src/zang/trigger.zig behind the same call shapes; `params` are opaque blobs of `params_size`
 * bytes (the Zig code is generic over NoteParamsType).  Slices returned by consume/dispatch stay
 * valid until the next call on the same object, like the Zig versions' internal arrays. */
typedef struct zh_impulse { uint64_t frame, note_id, event_id; } zh_impulse;                          /* notes.zig:58-62 */
typedef struct zh_iap { const zh_impulse *impulses; const void *paramses; uint64_t len; } zh_iap;     /* ImpulsesAndParamses :66-70 */
enum { ZH_MAX_IMPULSES = 32, ZH_MAX_PARAMS_SIZE = 64 };                                               /* notes.zig:73-74 */

typedef struct zh_impulse_queue zh_impulse_queue;                                                     /* notes.zig:72-128 */
ZH_API int zh_impulse_queue_create(uint32_t params_size, zh_impulse_queue **out);
ZH_API int zh_impulse_queue_destroy(zh_impulse_queue *q);
ZH_API int zh_impulse_queue_push(zh_impulse_queue *q, uint64_t impulse_frame, uint64_t note_id, const void *params);
ZH_API int zh_impulse_queue_consume(zh_impulse_queue *q, zh_iap *out);

typedef struct zh_note_tracker zh_note_tracker;                                                       /* notes.zig:138-207 */
/* song: n events, each {params blob, t (seconds, f32), note_id}; given as three parallel arrays (copied) */
ZH_API int zh_note_tracker_create(uint32_t params_size, uint64_t n_events, const void *paramses, const float *t,
                                  const uint64_t *note_ids, zh_note_tracker **out);
ZH_API int zh_note_tracker_destroy(zh_note_tracker *nt);
ZH_API int zh_note_tracker_reset(zh_note_tracker *nt);
ZH_API int zh_note_tracker_consume(zh_note_tracker *nt, float sample_rate, uint64_t span_start, uint64_t span_end, zh_iap *out);

typedef struct zh_polyphony_dispatcher zh_polyphony_dispatcher;                                       /* notes.zig:209-349 */
/* note_on is read from each params blob at byte `note_on_offset` (1 byte, non-zero = on) */
ZH_API int zh_polyphony_dispatcher_create(uint32_t polyphony, uint32_t params_size, uint32_t note_on_offset,
                                          zh_polyphony_dispatcher **out);
ZH_API int zh_polyphony_dispatcher_destroy(zh_polyphony_dispatcher *pd);
ZH_API int zh_polyphony_dispatcher_reset(zh_polyphony_dispatcher *pd);
ZH_API int zh_polyphony_dispatcher_dispatch(zh_polyphony_dispatcher *pd, zh_iap iap, zh_iap *out /*[polyphony]*/);

typedef struct zh_trigger zh_trigger;                                                                 /* trigger.zig:26-198 */
typedef struct zh_paint_span {                                                                        /* NewPaintReturnValue :50-54 */
    uint64_t start, end; uint32_t note_id_changed; uint32_t reserved; uint8_t params[64];
} zh_paint_span;
ZH_API int zh_trigger_create(uint32_t params_size, zh_trigger **out);
ZH_API int zh_trigger_destroy(zh_trigger *t);
ZH_API int zh_trigger_reset(zh_trigger *t);                                                           /* :62-64 */
ZH_API int zh_trigger_counter(zh_trigger *t, uint64_t span_start, uint64_t span_end, zh_iap iap);     /* :66-78 */
ZH_API int zh_trigger_next(zh_trigger *t, zh_paint_span *out);   /* :80-105; returns 1 = span produced, 0 = null, <0 error */

/* Voice(T)'s scheduling half (examples/example_song.zig:287-350): NoteTracker -> PolyphonyDispatcher(polyphony) ->
 * one Trigger per sub-voice.  zh_poly_voice_schedule makes the scheduling calls of `n_buffers` consecutive
 * Voice(T).paint invocations (buffer b has frames[b] frames; its sub-spans are shifted by the frames before it,
 * Trigger's carry-over splitting notes at every buffer edge exactly as per-buffer calls do) and records per
 * sub-voice the (span, params, note_id_changed) of every module.paint the reference would issue, laid out like
 * zh_span_table: [span][sub_voice], `max_spans` rows, counts[sub_voice].  ZH_ERR_INVALID if a list overflows. */
typedef struct zh_poly_voice zh_poly_voice;
ZH_API int zh_poly_voice_create(uint32_t polyphony, uint32_t params_size, uint32_t note_on_offset, uint64_t n_events,
                                const void *paramses, const float *t, const uint64_t *note_ids, zh_poly_voice **out);
ZH_API int zh_poly_voice_destroy(zh_poly_voice *pv);
ZH_API int zh_poly_voice_reset(zh_poly_voice *pv);
ZH_API int zh_poly_voice_schedule(zh_poly_voice *pv, float sample_rate, const uint32_t *frames, uint32_t n_buffers,
                                  uint32_t max_spans, uint32_t *counts, uint32_t *start, uint32_t *end, void *params,
                                  uint8_t *note_id_changed);

/* ---------------------------------------------------------------- voice bank: the same scheduling ON THE DEVICE
 * N independent instruments, each the scheduling half of Voice(T) with the same polyphony, their songs and all scheduler
 * state resident in device memory.  zh_voice_bank_schedule enqueues ONE kernel per 32 buffers on the context's stream that
 * advances every instrument and writes the [span][voice] tables the *_paint_spans entry points read (voice = instrument *
 * polyphony + slot): no host work per buffer beyond the launch, no sync, no copy.  Results equal zh_poly_voice_schedule's
 * per instrument, bit for bit (a 33rd impulse dropped, an event behind the clock on frame 0, the tracker's f32 arithmetic).
 * Songs are in CSR form: instrument i owns events [event_offsets[i], event_offsets[i + 1]) of paramses / t / note_ids
 * (copied once; event_offsets[0] == 0, fewer than 2^32 - 1 events in all).  Records are params_size bytes, a multiple of 4,
 * at most ZH_MAX_PARAMS_SIZE; note_on is the byte at note_on_offset.  The frames of one schedule call sum to less than 2^32.
 * OVERFLOW: a voice's list stops at max_spans (count == max_spans), its Trigger state still advances as if every sub-span
 * had been emitted, and a device counter is incremented per dropped sub-span: zh_voice_bank_overflows synchronises and
 * returns it (33 rows per buffer always suffice).
 * schedule never allocates: table capacity is 4 rows at creation, changed by zh_voice_bank_reserve (refused while a
 * capture records: ZH_ERR_UNSUPPORTED); max_spans above it is ZH_ERR_INVALID.  Table addresses stay fixed between reserve
 * calls, so a graph that holds schedule + paint can be replayed (`frames` is read when the call is made: a replay repeats
 * the same buffer lengths); a reserve that changes the capacity INVALIDATES views and graphs made before it.  Capturable;
 * under ZH_CAPTURE_COALESCE it records what was held back first.  Zero instruments: ZH_OK, nothing runs.
 * Views are device pointers into the bank's tables, no copy: zh_voice_bank_span_param gives record word `word` as both `f`
 * and `u` of one array (clear the one a field does not take); zh_voice_bank_span_table takes the word that holds freq. */
typedef struct zh_voice_bank zh_voice_bank;
typedef struct zh_voice_bank_instrument_state { uint64_t next_event; float t; uint32_t reserved; } zh_voice_bank_instrument_state;
typedef struct zh_voice_bank_voice_state {
    uint32_t used, note_on; uint64_t note_id, event_id;          /* the dispatcher's slot */
    uint32_t has_note, reserved; uint64_t trigger_note_id;       /* the Trigger's carried note ... */
    uint64_t trigger_event;                                      /* ... and the index of its event in the bank's arrays */
} zh_voice_bank_voice_state;
ZH_API int zh_voice_bank_create(zh_ctx *ctx, uint32_t n_instruments, uint32_t polyphony, uint32_t params_size, uint32_t note_on_offset,
                                const uint64_t *event_offsets, const void *paramses, const float *t, const uint64_t *note_ids,
                                zh_voice_bank **out);
ZH_API int zh_voice_bank_destroy(zh_voice_bank *bank);
ZH_API int zh_voice_bank_reset(zh_voice_bank *bank);                                                  /* example_song.zig:318-324 */
ZH_API int zh_voice_bank_reserve(zh_voice_bank *bank, uint32_t max_rows);
ZH_API int zh_voice_bank_schedule(zh_voice_bank *bank, float sample_rate, const uint32_t *frames, uint32_t n_buffers, uint32_t max_spans);
ZH_API int zh_voice_bank_script_table(const zh_voice_bank *bank, uint32_t max_spans, zh_script_span_table *out);
ZH_API int zh_voice_bank_span_param(const zh_voice_bank *bank, uint32_t word, zh_script_span_param *out);
ZH_API int zh_voice_bank_span_table(const zh_voice_bank *bank, uint32_t max_spans, uint32_t freq_word, zh_span_table *out);
ZH_API int zh_voice_bank_overflows(zh_voice_bank *bank, uint64_t *out);
ZH_API int zh_voice_bank_get_state(zh_voice_bank *bank, zh_voice_bank_instrument_state *instruments /*[n]*/,
                                   zh_voice_bank_voice_state *voices /*[n * polyphony]*/);
ZH_API int zh_voice_bank_set_state(zh_voice_bank *bank, const zh_voice_bank_instrument_state *instruments,
                                   const zh_voice_bank_voice_state *voices);

/* LIVE voice banks: the same tables from impulses pushed from outside (Notes(T).ImpulseQueue, notes.zig:72-128, as
 * examples/example_polyphony2.zig:61-95 uses it) instead of a song.  A live bank has no song; every call of
 * zh_voice_bank_schedule_live schedules ONE buffer [0, out_len) from one batch of pushes over all instruments, in push order:
 * per instrument exactly zh_impulse_queue_push for each of its entries in batch order, zh_impulse_queue_consume,
 * zh_polyphony_dispatcher_dispatch, then zh_trigger_counter(0, out_len) and zh_trigger_next per slot -- in one kernel
 * (k_voice_bank_schedule_live), bit for bit.  So: a push is dropped when 32 of that instrument are accepted in this call or when
 * its frame is below the last accepted one's; an accepted one takes event_id = next_event_id++ (per instrument, from 1, kept
 * across calls; zh_voice_bank_reset clears the dispatcher and the Triggers and leaves it alone: ImpulseQueue has no reset).
 * Where the reference says "not sure what would happen", what that composition gives: an impulse whose frame is >= out_len is
 * accepted, takes an event id and its slot in the dispatcher, ends a carried note at out_len like any later impulse, and is never
 * painted (the next call does not see it; the note the Trigger carries on is the one before it); out_len == 0 does the same for
 * every impulse of the call and emits no sub-span.  A Trigger's carried note is kept as its record (the batch is gone by the
 * next call).  Sub-span frames are relative to the buffer; counts start from 0 every call.
 * The call validates, sorts the batch by instrument on the host (stable), copies it through pinned staging owned by the bank
 * (a ring; the call waits only for a slot whose copy is still in flight) and enqueues one copy and one launch: no stream
 * synchronise, and the caller's arrays may be reused on return.  batch == NULL or n == 0: no pushes (carried notes still paint).
 * ZH_ERR_INVALID: a song bank here or a live bank in zh_voice_bank_schedule / _get_state / _set_state, an instrument index
 * >= n_instruments, batch->n > max_impulses_per_call, max_spans of 0 or above the capacity.  ZH_ERR_UNSUPPORTED while a capture
 * records (a replay would read host memory that has since changed).  destroy / reset / reserve / script_table / span_param /
 * span_table / overflows work as on a song bank; overflow is handled the same way. */
typedef struct zh_bank_impulses {                                /* host arrays, in push order over all instruments */
    uint32_t n; const uint32_t *instrument, *frame; const uint64_t *note_id; const void *paramses;   /* [n] each; [n][params_size] */
} zh_bank_impulses;
typedef struct zh_voice_bank_live_voice_state {
    uint32_t used, note_on; uint64_t note_id, event_id;          /* the dispatcher's slot */
    uint32_t has_note, reserved; uint64_t trigger_note_id;       /* the Trigger's carried note ... */
    uint32_t carried[16];                                        /* ... and its record (params_size / 4 words; zeros without a note) */
} zh_voice_bank_live_voice_state;
ZH_API int zh_voice_bank_create_live(zh_ctx *ctx, uint32_t n_instruments, uint32_t polyphony, uint32_t params_size, uint32_t note_on_offset,
                                     uint32_t max_impulses_per_call, zh_voice_bank **out);
ZH_API int zh_voice_bank_schedule_live(zh_voice_bank *bank, uint32_t out_len, uint32_t max_spans, const zh_bank_impulses *batch);
ZH_API int zh_voice_bank_live_get_state(zh_voice_bank *bank, uint64_t *next_event_id /*[n]*/,
                                        zh_voice_bank_live_voice_state *voices /*[n * polyphony]*/);
ZH_API int zh_voice_bank_live_set_state(zh_voice_bank *bank, const uint64_t *next_event_id, const zh_voice_bank_live_voice_state *voices);

/* ---------------------------------------------------------------- single-voice host-pointer wrappers
 * The literal one-voice form of a Zig module call: `state` is the Zig struct (in/out), `outputs[0]` and every
 * input buffer are HOST float[>= span_end] slices exactly like zang's []f32, params are plain values.  Each call
 * stages through the device (upload, one-voice paint, download) and is synchronous: a drop-in for porting and
 * for checking a Zig caller against the GPU path, not a fast path (use the batched entry points for speed). */
typedef struct zh_hcob { uint32_t tag; float constant; const float *buffer; } zh_hcob;   /* host ConstantOrBuffer */
typedef struct zh_hcurve { uint32_t tag; float duration; } zh_hcurve;                     /* host PaintCurve */

typedef struct zh_sineosc_host_params { float sample_rate; zh_hcob freq, phase; } zh_sineosc_host_params;
typedef struct zh_pulseosc_host_params { float sample_rate; zh_hcob freq; float color; } zh_pulseosc_host_params;
typedef zh_pulseosc_host_params zh_trisawosc_host_params;
typedef struct zh_noise_host_params { uint32_t color; } zh_noise_host_params;
typedef struct zh_envelope_host_params { float sample_rate; zh_hcurve attack, decay, release; float sustain_volume; uint32_t note_on; } zh_envelope_host_params;
typedef struct zh_gate_host_params { uint32_t note_on; } zh_gate_host_params;
typedef struct zh_filter_host_params { const float *input; uint32_t type; zh_hcob cutoff, res; } zh_filter_host_params;
typedef struct zh_sampler_host_params {
    float sample_rate; uint64_t num_channels, sample_rate_in; uint32_t format; const uint8_t *data; uint64_t data_len;
    uint64_t channel; uint32_t loop;
} zh_sampler_host_params;
typedef struct zh_decimator_host_params { float sample_rate; const float *input; float fake_sample_rate; } zh_decimator_host_params;
typedef struct zh_distortion_host_params { const float *input; uint32_t type; float ingain, outgain, offset; } zh_distortion_host_params;

/* init() of the two modules whose Zig init() is not all-zeros (host side, no GPU work) */
ZH_API int zh_noise_state_init(zh_noise_state *state, uint64_t seed);          /* Noise.zig:25-32 with an explicit seed */
ZH_API int zh_decimator_state_init(zh_decimator_state *state);                  /* Decimator.zig:14-19 */

ZH_API int zh_sineosc_paint_host(zh_ctx *ctx, zh_sineosc_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_sineosc_host_params *params);
ZH_API int zh_pulseosc_paint_host(zh_ctx *ctx, zh_pulseosc_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_pulseosc_host_params *params);
ZH_API int zh_trisawosc_paint_host(zh_ctx *ctx, zh_trisawosc_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_trisawosc_host_params *params);
ZH_API int zh_noise_paint_host(zh_ctx *ctx, zh_noise_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_noise_host_params *params);
ZH_API int zh_envelope_paint_host(zh_ctx *ctx, zh_envelope_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_envelope_host_params *params);
ZH_API int zh_gate_paint_host(zh_ctx *ctx, void *state_unused, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_gate_host_params *params);
ZH_API int zh_filter_paint_host(zh_ctx *ctx, zh_filter_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_filter_host_params *params);
ZH_API int zh_sampler_paint_host(zh_ctx *ctx, zh_sampler_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_sampler_host_params *params);
ZH_API int zh_decimator_paint_host(zh_ctx *ctx, zh_decimator_state *state, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_decimator_host_params *params);
ZH_API int zh_distortion_paint_host(zh_ctx *ctx, void *state_unused, uint32_t span_start, uint32_t span_end, float *const *outputs, float *const *temps, uint32_t note_id_changed, const zh_distortion_host_params *params);

#ifdef __cplusplus
}
#endif
#endif /* ZANG_HIP_H */
