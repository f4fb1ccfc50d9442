// zang_hip.hpp -- C++17 host-side mirror of zang's `zang` and `modules` namespaces over the C ABI of
// include/zang_hip.h (header-only; link with -lzang_hip).
//
// The reference is Zig and its toolchain is absent from the build image, so the compiled-language host
// side above the C ABI is this header: the same names, argument order and meaning as the Zig code
//     module.paint(span, outputs, temps, note_id_changed, params)          (src/modules/SineOsc.zig:24-31)
//     zang.zero(span, buf) / zang.multiply(span, dest, a, b) / ...          (src/zang/basics.zig:12-78)
// with one difference of kind: a module object is a BATCH of n voices on the GPU and a buffer is a device
// image [frame][voice] (zang::Image) instead of a host []f32.  Errors: the Zig paint functions cannot fail;
// here a non-zero return of the C ABI throws zang::Error.  bindings/zang_hip.zig is the same thing for a
// Zig host; zang_amd/zang.py + modules.py for Python.  tests/cpp/host_parity.cpp uses this header the way
// examples/modules.zig uses zang.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "zang_hip.h"

namespace zang {

struct Error : std::runtime_error {
    int code;
    Error(int rc, const std::string &what) : std::runtime_error(what + ": " + zh_error_string(rc) + " (" + std::to_string(rc) + ")"), code(rc) {}
};
inline void check(int rc, const char *what) {
    if (rc != 0) throw Error(rc, what);
}

struct Span {                                   // src/zang/basics.zig:3-10
    uint32_t start, end;
    static Span init(uint32_t start, uint32_t end) { return Span{start, end}; }
};

class Context {
    zh_ctx *h_ = nullptr;

public:
    explicit Context(int device = 0) { check(zh_create(&h_, device), "zh_create"); }
    ~Context() { if (h_) zh_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    zh_ctx *get() const { return h_; }
    void sync() { check(zh_sync(h_), "zh_sync"); }
};

// The multi-GPU exchange as a collective (zh_comm_*: RCCL over xGMI, one rank per process, enqueued on the context's
// stream).  `id` = the 128 bytes rank 0 obtained from Comm::uniqueId() and handed to the other processes over any host
// channel; the constructor blocks until all `world` ranks have called it.
class Comm {
    zh_comm *h_ = nullptr;

public:
    using Id = std::array<uint8_t, ZH_COMM_ID_BYTES>;
    static bool available() { return zh_comm_available() == 1; }
    static Id uniqueId() { Id id{}; check(zh_comm_unique_id(id.data()), "zh_comm_unique_id"); return id; }
    Comm(Context &c, uint32_t world, uint32_t rank, const Id &id) { check(zh_comm_create(c.get(), world, rank, id.data(), &h_), "zh_comm_create"); }
    ~Comm() { if (h_) zh_comm_destroy(h_); }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    zh_comm *get() const { return h_; }
    void allreduceMix(float *mix_dev, size_t n) { check(zh_allreduce_mix(h_, mix_dev, n), "zh_allreduce_mix"); }
    void reduceMix(float *mix_dev, size_t n, uint32_t root) { check(zh_reduce_mix(h_, mix_dev, n, root), "zh_reduce_mix"); }
};

// A device sample image [frame][voice]: column v is what the reference calls one `[]f32` of voice v.
class Image {
    Context &ctx_;
    zh_buf b_{};

public:
    Image(Context &ctx, uint32_t voices, uint32_t frames) : ctx_(ctx) { check(zh_buf_alloc(ctx.get(), &b_, voices, frames), "zh_buf_alloc"); }
    ~Image() { zh_buf_free(ctx_.get(), &b_); }
    Image(const Image &) = delete;
    Image &operator=(const Image &) = delete;
    operator zh_buf() const { return b_; }
    uint32_t voices() const { return b_.voices; }
    uint32_t frames() const { return b_.frames; }
    // host layout: one contiguous []f32 per voice ([voice][frame])
    void upload(const std::vector<float> &voice_major) { check(zh_buf_upload_voices(ctx_.get(), b_, voice_major.data(), b_.frames), "zh_buf_upload_voices"); }
    std::vector<float> download() const {
        std::vector<float> out((size_t)b_.voices * b_.frames);
        check(zh_buf_download_voices(ctx_.get(), out.data(), b_, b_.frames), "zh_buf_download_voices");
        return out;
    }
};

// A device array of per-voice parameters (f32 or bool-as-u8).
template <class T> class DeviceArray {
    Context &ctx_;
    T *p_ = nullptr;
    size_t n_;

public:
    DeviceArray(Context &ctx, const std::vector<T> &host) : ctx_(ctx), n_(host.size()) {
        check(zh_malloc(ctx.get(), reinterpret_cast<void **>(&p_), n_ * sizeof(T)), "zh_malloc");
        check(zh_upload(ctx.get(), p_, host.data(), n_ * sizeof(T)), "zh_upload");
    }
    ~DeviceArray() { zh_free(ctx_.get(), p_); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    const T *get() const { return p_; }
    T *get() { return p_; }
    size_t size() const { return n_; }
    std::vector<T> download() const {
        std::vector<T> host(n_);
        check(zh_download(ctx_.get(), host.data(), p_, n_ * sizeof(T)), "zh_download");
        return host;
    }
};

// ---- values
inline zh_f32 f32(float v) { return zh_f32{v, 0, nullptr}; }
inline zh_f32 f32(const DeviceArray<float> &per_voice) { return zh_f32{0.0f, 0, per_voice.get()}; }
inline zh_u32 u32(uint32_t v) { return zh_u32{v, 0, nullptr}; }
inline zh_u32 u32(const DeviceArray<uint32_t> &per_voice) { return zh_u32{0, 0, per_voice.get()}; }
inline zh_bool boolean(bool v) { return zh_bool{v ? 1u : 0u, 0, nullptr}; }
inline zh_bool boolean(const DeviceArray<uint8_t> &per_voice) { return zh_bool{0, 0, per_voice.get()}; }

// zang.constant / zang.buffer (src/zang/constant_or_buffer.zig:9-15)
inline zh_cob constant(float v) { return zh_cob{ZH_COB_CONSTANT, 0, f32(v), zh_buf{}}; }
inline zh_cob constant(const DeviceArray<float> &per_voice) { return zh_cob{ZH_COB_CONSTANT, 0, f32(per_voice), zh_buf{}}; }
inline zh_cob buffer(const zh_buf &b) { return zh_cob{ZH_COB_BUFFER, 0, zh_f32{}, b}; }

// zang.PaintCurve (src/zang/painter.zig:25-30)
struct PaintCurve {
    static zh_curve instantaneous() { return zh_curve{ZH_CURVE_INSTANTANEOUS, 0, f32(0.0f)}; }
    static zh_curve linear(float d) { return zh_curve{ZH_CURVE_LINEAR, 0, f32(d)}; }
    static zh_curve squared(float d) { return zh_curve{ZH_CURVE_SQUARED, 0, f32(d)}; }
    static zh_curve cubed(float d) { return zh_curve{ZH_CURVE_CUBED, 0, f32(d)}; }
};

// ---- basics.zig:12-78 (same names, `span` first)
inline void zero(Context &c, Span s, zh_buf dest) { check(zh_zero(c.get(), s.start, s.end, dest), "zero"); }
inline void set(Context &c, Span s, zh_buf dest, float a) { check(zh_set(c.get(), s.start, s.end, dest, f32(a)), "set"); }
inline void copy(Context &c, Span s, zh_buf dest, zh_buf src) { check(zh_copy(c.get(), s.start, s.end, dest, src), "copy"); }
inline void add(Context &c, Span s, zh_buf dest, zh_buf a, zh_buf b) { check(zh_add(c.get(), s.start, s.end, dest, a, b), "add"); }
inline void addInto(Context &c, Span s, zh_buf dest, zh_buf src) { check(zh_add_into(c.get(), s.start, s.end, dest, src), "addInto"); }
inline void addScalar(Context &c, Span s, zh_buf dest, zh_buf a, float b) { check(zh_add_scalar(c.get(), s.start, s.end, dest, a, f32(b)), "addScalar"); }
inline void addScalarInto(Context &c, Span s, zh_buf dest, float a) { check(zh_add_scalar_into(c.get(), s.start, s.end, dest, f32(a)), "addScalarInto"); }
inline void multiply(Context &c, Span s, zh_buf dest, zh_buf a, zh_buf b) { check(zh_multiply(c.get(), s.start, s.end, dest, a, b), "multiply"); }
inline void multiplyWith(Context &c, Span s, zh_buf dest, zh_buf a) { check(zh_multiply_with(c.get(), s.start, s.end, dest, a), "multiplyWith"); }
inline void multiplyScalar(Context &c, Span s, zh_buf dest, zh_buf a, float b) { check(zh_multiply_scalar(c.get(), s.start, s.end, dest, a, f32(b)), "multiplyScalar"); }
inline void multiplyWithScalar(Context &c, Span s, zh_buf dest, float a) { check(zh_multiply_with_scalar(c.get(), s.start, s.end, dest, f32(a)), "multiplyWithScalar"); }

// the sum of all voices of an image: dst_dev[f] (+)= sum_v src[f][v] (V x zang.addInto, basics.zig:31-36; fixed-order tree sum)
inline void mixdownVoices(Context &c, Span s, float *dst_dev, zh_buf src, uint32_t flags = ZH_PAINT_ADD) {
    check(zh_mixdown_voices(c.get(), s.start, s.end, dst_dev, src, flags), "mixdownVoices");
}
// zang.mixDown (src/zang/mixdown.zig:8-86): f32 mix -> interleaved s8 / s16 LE PCM with clamping, on the device
inline void mixDown(Context &c, uint8_t *dst_dev, const float *mix_dev, uint32_t n, uint32_t audio_format, uint32_t num_channels,
                    uint32_t channel_index, float vol) {
    check(zh_mix_down(c.get(), dst_dev, mix_dev, n, audio_format, num_channels, channel_index, vol), "mixDown");
}
// every group of `group_voices` consecutive voices of an image on its own, added in voice order (the bits of successive `+=`
// paints): dst_dev[g * dst_stride_floats + f] (+)= src[f][g*P] + ... + src[f][g*P + P-1], all groups in one launch
inline void mixdownGroups(Context &c, Span s, float *dst_dev, size_t dst_stride_floats, zh_buf src, uint32_t group_voices,
                          uint32_t flags = ZH_PAINT_ADD) {
    check(zh_mixdown_groups(c.get(), s.start, s.end, dst_dev, dst_stride_floats, src, group_voices, flags), "mixdownGroups");
}
// the same sums (starting from acc_dev's rows, or from 0 when it is null) straight through zang.mixDown into one PCM row per group
inline void mixdownGroupsPcm(Context &c, Span s, uint8_t *dst_dev, size_t dst_stride_bytes, zh_buf src, uint32_t group_voices,
                             const float *acc_dev, size_t acc_stride_floats, uint32_t audio_format, uint32_t num_channels,
                             uint32_t channel_index, float vol) {
    check(zh_mixdown_groups_pcm(c.get(), s.start, s.end, dst_dev, dst_stride_bytes, src, group_voices, acc_dev, acc_stride_floats, audio_format,
                                num_channels, channel_index, vol), "mixdownGroupsPcm");
}

// A voice bank (zh_voice_bank_*): n instruments' NoteTracker -> PolyphonyDispatcher(polyphony) -> Triggers on the device
// (examples/example_song.zig:287-350 without the paints).  schedule() enqueues the kernel that fills the span tables; the
// views hand them to a module's paint_spans / zh_nice_paint_spans as device pointers.  Record = the song's NoteParamsType
// (trivially copyable, sizeof a multiple of 4, at most 64 bytes); instrument i owns events [offsets[i], offsets[i + 1]).
class VoiceBank {
    zh_voice_bank *h_ = nullptr;
    uint32_t n_, polyphony_;

public:
    template <class Record>
    VoiceBank(Context &ctx, uint32_t polyphony, uint32_t note_on_offset, const std::vector<uint64_t> &offsets, const std::vector<Record> &records,
              const std::vector<float> &t, const std::vector<uint64_t> &note_ids)
        : n_(offsets.empty() ? 0u : (uint32_t)(offsets.size() - 1)), polyphony_(polyphony) {
        if (records.size() != t.size() || note_ids.size() != t.size() || (n_ && offsets.back() != t.size()))
            throw Error(ZH_ERR_INVALID, "VoiceBank: one record, one time and one note id per event");
        check(zh_voice_bank_create(ctx.get(), n_, polyphony, (uint32_t)sizeof(Record), note_on_offset, n_ ? offsets.data() : nullptr, records.data(),
                                   t.data(), note_ids.data(), &h_), "zh_voice_bank_create");
    }
    ~VoiceBank() { if (h_) zh_voice_bank_destroy(h_); }
    VoiceBank(const VoiceBank &) = delete;
    VoiceBank &operator=(const VoiceBank &) = delete;
    zh_voice_bank *get() const { return h_; }
    uint32_t instruments() const { return n_; }
    uint32_t voices() const { return n_ * polyphony_; }
    void reset() { check(zh_voice_bank_reset(h_), "zh_voice_bank_reset"); }
    void reserve(uint32_t max_rows) { check(zh_voice_bank_reserve(h_, max_rows), "zh_voice_bank_reserve"); }   // invalidates views and graphs
    void schedule(float sample_rate, const std::vector<uint32_t> &frames, uint32_t max_spans) {
        check(zh_voice_bank_schedule(h_, sample_rate, frames.data(), (uint32_t)frames.size(), max_spans), "zh_voice_bank_schedule");
    }
    zh_script_span_table scriptTable(uint32_t max_spans) const {
        zh_script_span_table t{};
        check(zh_voice_bank_script_table(h_, max_spans, &t), "zh_voice_bank_script_table");
        return t;
    }
    zh_script_span_param spanParamF(uint32_t word) const { zh_script_span_param p = spanParam(word); p.u = nullptr; return p; }
    zh_script_span_param spanParamU(uint32_t word) const { zh_script_span_param p = spanParam(word); p.f = nullptr; return p; }
    zh_span_table spanTable(uint32_t max_spans, uint32_t freq_word) const {
        zh_span_table t{};
        check(zh_voice_bank_span_table(h_, max_spans, freq_word, &t), "zh_voice_bank_span_table");
        return t;
    }
    uint64_t overflows() { uint64_t n = 0; check(zh_voice_bank_overflows(h_, &n), "zh_voice_bank_overflows"); return n; }
    struct State { std::vector<zh_voice_bank_instrument_state> instruments; std::vector<zh_voice_bank_voice_state> voices; };
    State getState() {
        State s{std::vector<zh_voice_bank_instrument_state>(n_), std::vector<zh_voice_bank_voice_state>(voices())};
        check(zh_voice_bank_get_state(h_, s.instruments.data(), s.voices.data()), "zh_voice_bank_get_state");
        return s;
    }
    void setState(const State &s) {
        if (s.instruments.size() != n_ || s.voices.size() != voices()) throw Error(ZH_ERR_INVALID, "VoiceBank::setState: a state of another bank");
        check(zh_voice_bank_set_state(h_, s.instruments.data(), s.voices.data()), "zh_voice_bank_set_state");
    }

private:
    zh_script_span_param spanParam(uint32_t word) const {
        zh_script_span_param p{};
        check(zh_voice_bank_span_param(h_, word, &p), "zh_voice_bank_span_param");
        return p;
    }
};

// A live voice bank (zh_voice_bank_create_live): no song; push() collects impulses on the host as Notes(T).ImpulseQueue.push does
// (examples/example_polyphony2.zig:80-95), schedule() sends them and enqueues the kernel that takes every instrument through
// ImpulseQueue -> PolyphonyDispatcher -> Triggers for one buffer.  Views as on VoiceBank.
template <class Record>
class LiveVoiceBank {
    static_assert(sizeof(Record) % 4 == 0 && sizeof(Record) <= ZH_MAX_PARAMS_SIZE, "a record is a multiple of 4 bytes, at most 64");
    zh_voice_bank *h_ = nullptr;
    uint32_t n_, polyphony_;
    std::vector<uint32_t> instrument_, frame_;
    std::vector<uint64_t> note_id_;
    std::vector<Record> records_;

public:
    LiveVoiceBank(Context &ctx, uint32_t n_instruments, uint32_t polyphony, uint32_t note_on_offset, uint32_t max_impulses)
        : n_(n_instruments), polyphony_(polyphony) {
        check(zh_voice_bank_create_live(ctx.get(), n_instruments, polyphony, (uint32_t)sizeof(Record), note_on_offset, max_impulses, &h_),
              "zh_voice_bank_create_live");
    }
    ~LiveVoiceBank() { if (h_) zh_voice_bank_destroy(h_); }
    LiveVoiceBank(const LiveVoiceBank &) = delete;
    LiveVoiceBank &operator=(const LiveVoiceBank &) = delete;
    zh_voice_bank *get() const { return h_; }
    uint32_t instruments() const { return n_; }
    uint32_t voices() const { return n_ * polyphony_; }
    void reset() { check(zh_voice_bank_reset(h_), "zh_voice_bank_reset"); }
    void reserve(uint32_t max_rows) { check(zh_voice_bank_reserve(h_, max_rows), "zh_voice_bank_reserve"); }   // invalidates views
    void push(uint32_t instrument, uint32_t frame, uint64_t note_id, const Record &record) {
        instrument_.push_back(instrument); frame_.push_back(frame); note_id_.push_back(note_id); records_.push_back(record);
    }
    void schedule(uint32_t out_len, uint32_t max_spans) {          // what was pushed since the last call; the lists are empty afterwards
        const zh_bank_impulses batch{(uint32_t)instrument_.size(), instrument_.data(), frame_.data(), note_id_.data(), records_.data()};
        const int rc = zh_voice_bank_schedule_live(h_, out_len, max_spans, batch.n ? &batch : nullptr);
        instrument_.clear(); frame_.clear(); note_id_.clear(); records_.clear();
        check(rc, "zh_voice_bank_schedule_live");
    }
    zh_script_span_table scriptTable(uint32_t max_spans) const {
        zh_script_span_table t{};
        check(zh_voice_bank_script_table(h_, max_spans, &t), "zh_voice_bank_script_table");
        return t;
    }
    zh_script_span_param spanParamF(uint32_t word) const { zh_script_span_param p = spanParam(word); p.u = nullptr; return p; }
    zh_script_span_param spanParamU(uint32_t word) const { zh_script_span_param p = spanParam(word); p.f = nullptr; return p; }
    zh_span_table spanTable(uint32_t max_spans, uint32_t freq_word) const {
        zh_span_table t{};
        check(zh_voice_bank_span_table(h_, max_spans, freq_word, &t), "zh_voice_bank_span_table");
        return t;
    }
    uint64_t overflows() { uint64_t n = 0; check(zh_voice_bank_overflows(h_, &n), "zh_voice_bank_overflows"); return n; }
    struct State { std::vector<uint64_t> next_event_id; std::vector<zh_voice_bank_live_voice_state> voices; };
    State getState() {
        State s{std::vector<uint64_t>(n_), std::vector<zh_voice_bank_live_voice_state>(voices())};
        check(zh_voice_bank_live_get_state(h_, s.next_event_id.data(), s.voices.data()), "zh_voice_bank_live_get_state");
        return s;
    }
    void setState(const State &s) {
        if (s.next_event_id.size() != n_ || s.voices.size() != voices()) throw Error(ZH_ERR_INVALID, "LiveVoiceBank::setState: a state of another bank");
        check(zh_voice_bank_live_set_state(h_, s.next_event_id.data(), s.voices.data()), "zh_voice_bank_live_set_state");
    }

private:
    zh_script_span_param spanParam(uint32_t word) const {
        zh_script_span_param p{};
        check(zh_voice_bank_span_param(h_, word, &p), "zh_voice_bank_span_param");
        return p;
    }
};

// The FM synth voice of examples/example_fmsynth.zig (:22-356) for n_voices voices, `group` consecutive ones per instrument (a synth's
// polyphony: one patch and one column of the LFO images each).  paint / paintSpans as on the fused composites below; flags may
// carry ZH_FM_SPLIT_OPERATORS (outputs[0] then has 2 * n_voices columns: the modulator's and the carrier's part of every voice).
class FMInstrument {
    zh_fm *h_ = nullptr;
    uint32_t n_, group_;

public:
    static constexpr size_t num_outputs = 1;
    static constexpr size_t num_temps = 3;
    using Params = zh_fm_params;
    using Patch = zh_fm_patch;
    FMInstrument(Context &ctx, uint32_t n_voices, uint32_t group = 1) : n_(n_voices), group_(group) {
        check(zh_fm_create(ctx.get(), n_voices, group, &h_), "zh_fm_create");
    }
    ~FMInstrument() { if (h_) zh_fm_destroy(h_); }
    FMInstrument(const FMInstrument &) = delete;
    FMInstrument &operator=(const FMInstrument &) = delete;
    zh_fm *get() const { return h_; }
    uint32_t voices() const { return n_; }
    uint32_t instruments() const { return group_ ? (n_ + group_ - 1) / group_ : 0; }
    static Patch defaultPatch() { Patch p{}; check(zh_fm_patch_default(&p), "zh_fm_patch_default"); return p; }   // :376-397
    // one patch for every instrument, or one per instrument; a value outside its num_values is refused and nothing changes
    void setPatches(const std::vector<Patch> &patches) { check(zh_fm_set_patches(h_, patches.data(), (uint32_t)patches.size()), "zh_fm_set_patches"); }
    std::vector<zh_fm_state> getState() {
        std::vector<zh_fm_state> s(n_);
        check(zh_fm_get_state(h_, s.data()), "zh_fm_get_state");
        return s;
    }
    void setState(const std::vector<zh_fm_state> &s) {
        if (s.size() != n_) throw Error(ZH_ERR_INVALID, "FMInstrument::setState: a state of another instrument");
        check(zh_fm_set_state(h_, s.data()), "zh_fm_set_state");
    }
    void paint(Span span, const std::array<zh_buf, 1> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_fm_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_fm_paint");
    }
    // the synth's Trigger loop (:457-496) for every voice in one call; `table`: uploaded by the host, or a voice bank's spanTable()
    void paintSpans(Span span, const std::array<zh_buf, 1> &outputs, float sample_rate, const zh_buf &tremolo_input, const zh_buf &vibrato_input,
                    const zh_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_fm_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, sample_rate, tremolo_input, vibrato_input, &table, flags),
              "zh_fm_paint_spans");
    }
};

// K samples resident on the device (zh_sample_kit): `samples[i].data` are HOST pointers here, copied once; sample(i) hands entry i
// back with its DEVICE pointer, for the plain Sampler paints.  Destroy it before its context.
class SampleKit {
    zh_sample_kit *h_ = nullptr;

public:
    SampleKit(Context &ctx, const std::vector<zh_sample> &samples) {
        check(zh_sample_kit_create(ctx.get(), samples.data(), (uint32_t)samples.size(), &h_), "zh_sample_kit_create");
    }
    ~SampleKit() { if (h_) zh_sample_kit_destroy(h_); }
    SampleKit(const SampleKit &) = delete;
    SampleKit &operator=(const SampleKit &) = delete;
    zh_sample_kit *get() const { return h_; }
    uint32_t count() const { uint32_t n = 0; check(zh_sample_kit_count(h_, &n), "zh_sample_kit_count"); return n; }
    zh_sample sample(uint32_t i) const { zh_sample s{}; check(zh_sample_kit_sample(h_, i, &s), "zh_sample_kit_sample"); return s; }
};

// K sound effects resident on the device (zh_sfx_kit), each three curves: `effects[i].<curve>.nodes` are HOST pointers here, copied
// once; effect(i) hands entry i back with DEVICE pointers, for zh_curve_module_paint.  Destroy it before its context.
class SfxKit {
    zh_sfx_kit *h_ = nullptr;

public:
    SfxKit(Context &ctx, const std::vector<zh_sfx_effect> &effects) {
        check(zh_sfx_kit_create(ctx.get(), effects.data(), (uint32_t)effects.size(), &h_), "zh_sfx_kit_create");
    }
    ~SfxKit() { if (h_) zh_sfx_kit_destroy(h_); }
    SfxKit(const SfxKit &) = delete;
    SfxKit &operator=(const SfxKit &) = delete;
    zh_sfx_kit *get() const { return h_; }
    uint32_t count() const { uint32_t n = 0; check(zh_sfx_kit_count(h_, &n), "zh_sfx_kit_count"); return n; }
    zh_sfx_effect effect(uint32_t i) const { zh_sfx_effect e{}; check(zh_sfx_kit_effect(h_, i, &e), "zh_sfx_kit_effect"); return e; }
};

// LaserPlayer (examples/example_laser.zig:40-117) for n voices as one fused kernel; the curves come from an SfxKit
class Laser {
    zh_laser *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 1;
    static constexpr size_t num_temps = 3;
    using Params = zh_laser_params;
    using State = zh_laser_state;
    Laser(Context &ctx, uint32_t n_voices) { check(zh_laser_create(ctx.get(), n_voices, &h_), "zh_laser_create"); }
    ~Laser() { if (h_) zh_laser_destroy(h_); }
    Laser(const Laser &) = delete;
    Laser &operator=(const Laser &) = delete;
    zh_laser *get() const { return h_; }
    void getState(State *host) const { check(zh_laser_get_state(h_, host), "zh_laser_get_state"); }
    void setState(const State *host) { check(zh_laser_set_state(h_, host), "zh_laser_set_state"); }
    void paint(Span span, const std::array<zh_buf, 1> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_laser_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_laser_paint");
    }
    // MainModule's Trigger loop (:149-158) for every voice in one call; span_params = host array [ZH_LASER_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 1> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_laser_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_laser_paint_spans");
    }
};

// OuterInstrument over Instrument (examples/example_detuned.zig:31-169) for n voices as one fused kernel: outputs[0] = the voice,
// outputs[1] = the frequency image (a zh_buf{} whose ptr is NULL: not painted); voice v's noise is seeded with first_seed + v
class Detuned {
    zh_detuned *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 2;
    static constexpr size_t num_temps = 4;
    using Params = zh_detuned_params;
    using Patch = zh_detuned_patch;
    using State = zh_detuned_state;
    Detuned(Context &ctx, uint32_t n_voices, uint64_t first_seed = 0) { check(zh_detuned_create(ctx.get(), n_voices, first_seed, &h_), "zh_detuned_create"); }
    ~Detuned() { if (h_) zh_detuned_destroy(h_); }
    Detuned(const Detuned &) = delete;
    Detuned &operator=(const Detuned &) = delete;
    zh_detuned *get() const { return h_; }
    static Patch defaultPatch() { Patch p{}; check(zh_detuned_patch_default(&p), "zh_detuned_patch_default"); return p; }
    void getState(State *host) const { check(zh_detuned_get_state(h_, host), "zh_detuned_get_state"); }
    void setState(const State *host) { check(zh_detuned_set_state(h_, host), "zh_detuned_set_state"); }
    void paint(Span span, const std::array<zh_buf, 2> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_detuned_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_detuned_paint");
    }
    // MainModule's Trigger loop (:213-222) for every voice in one call; span_params = host array [ZH_DETUNED_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 2> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_detuned_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_detuned_paint_spans");
    }
};

// CurvePlayer (examples/example_curve.zig:33-96) for n voices as one fused kernel: outputs[0] = the voice, outputs[1] = the carrier's
// frequency image (a zh_buf{} whose ptr is NULL: not painted); the modulator and carrier curves come from an SfxKit
class CurvePlayer {
    zh_curve_player *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 2;
    static constexpr size_t num_temps = 2;
    using Params = zh_curve_player_params;
    using State = zh_curve_player_state;
    CurvePlayer(Context &ctx, uint32_t n_voices) { check(zh_curve_player_create(ctx.get(), n_voices, &h_), "zh_curve_player_create"); }
    ~CurvePlayer() { if (h_) zh_curve_player_destroy(h_); }
    CurvePlayer(const CurvePlayer &) = delete;
    CurvePlayer &operator=(const CurvePlayer &) = delete;
    zh_curve_player *get() const { return h_; }
    void getState(State *host) const { check(zh_curve_player_get_state(h_, host), "zh_curve_player_get_state"); }
    void setState(const State *host) { check(zh_curve_player_set_state(h_, host), "zh_curve_player_set_state"); }
    void paint(Span span, const std::array<zh_buf, 2> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_curve_player_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_curve_player_paint");
    }
    // MainModule's Trigger loop (:126-129) for every voice in one call; span_params = host array [ZH_CURVE_PLAYER_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 2> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_curve_player_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags),
              "zh_curve_player_paint_spans");
    }
};

// fft(N, re, im) of examples/common/fft.zig (:25-60) for every voice, in place on rows [frame_start, frame_start + n) of both images
inline void fft(Context &c, uint32_t n, zh_buf re, zh_buf im, uint32_t frame_start = 0) { check(zh_fft(c.get(), n, frame_start, re, im), "fft"); }

// DrawSpectrum.plot (examples/visual.zig:257-280) for n voices: fft_out as a [512][voice] image, assigned by every plot
class Spectrum {
    Context &ctx_;
    Image out_;

public:
    Spectrum(Context &ctx, uint32_t n_voices) : ctx_(ctx), out_(ctx, n_voices, 512) { zero(ctx, Span{0, 512}, out_); }   // :245
    const Image &plot(zh_buf samples, uint32_t frame_start = 0) {
        check(zh_spectrum_plot(ctx_.get(), frame_start, samples, out_), "zh_spectrum_plot");
        return out_;
    }
    const Image &out() const { return out_; }
};

// DrawSpectrumFull (examples/visual.zig:363-458) for n voices: a [height][width][voice] buffer of pixel words on the device, one
// column per plot at drawindex, which wraps at width; a change of `logarithmic` zeroes the buffer and resets drawindex first
class Spectrogram {
    Context &ctx_;
    uint32_t voices_, width_, height_, drawindex_ = 0;
    bool logarithmic_ = false;
    DeviceArray<uint32_t> buffer_;

public:
    Spectrogram(Context &ctx, uint32_t n_voices, uint32_t width, uint32_t height)
        : ctx_(ctx), voices_(n_voices), width_(width), height_(height), buffer_(ctx, std::vector<uint32_t>((size_t)height * width * n_voices, 0u)) {
        if (height < 2 || width < 1) throw Error(ZH_ERR_INVALID, "Spectrogram: height >= 2 and width >= 1");
    }
    uint32_t drawindex() const { return drawindex_; }
    bool logarithmic() const { return logarithmic_; }
    void plot(zh_buf samples, uint32_t frame_start, bool logarithmic) {                                                   // :411-452
        if (logarithmic_ != logarithmic) {
            logarithmic_ = logarithmic;
            const std::vector<uint32_t> zeros(buffer_.size(), 0u);
            check(zh_upload(ctx_.get(), buffer_.get(), zeros.data(), zeros.size() * sizeof(uint32_t)), "zh_upload");
            drawindex_ = 0;
        }
        check(zh_spectrum_column(ctx_.get(), frame_start, samples, buffer_.get() + (size_t)drawindex_ * voices_, (size_t)width_ * voices_, height_,
                                 logarithmic ? 1 : 0), "zh_spectrum_column");
        if (++drawindex_ == width_) drawindex_ = 0;
    }
    std::vector<uint32_t> download() const { return buffer_.download(); }                     // [height][width][voice] as stored
    // the picture in time order, as scrollBlit (:127-139) draws it: stored columns drawindex.. first, then ..drawindex
    std::vector<uint32_t> scrolled() const {
        const std::vector<uint32_t> b = buffer_.download();
        std::vector<uint32_t> out(b.size());
        for (uint32_t y = 0; y < height_; y++)
            for (uint32_t x = 0; x < width_; x++)
                for (uint32_t v = 0; v < voices_; v++)
                    out[((size_t)y * width_ + x) * voices_ + v] = b[((size_t)y * width_ + (x + drawindex_) % width_) * voices_ + v];
        return out;
    }
};

// Instrument of examples/example_portamento.zig (:20-87) for n voices as one fused kernel: a sine whose frequency glides toward
// the note's, times an envelope; the voice carries prev_note_on across sub-spans.  outputs[0] = the voice, outputs[1] = the
// frequency image (a zh_buf{} whose ptr is NULL: not painted)
class Porta {
    zh_porta *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 2;
    static constexpr size_t num_temps = 3;
    using Params = zh_porta_params;
    using Patch = zh_porta_patch;
    using State = zh_porta_state;
    Porta(Context &ctx, uint32_t n_voices) { check(zh_porta_create(ctx.get(), n_voices, &h_), "zh_porta_create"); }
    ~Porta() { if (h_) zh_porta_destroy(h_); }
    Porta(const Porta &) = delete;
    Porta &operator=(const Porta &) = delete;
    zh_porta *get() const { return h_; }
    static Patch defaultPatch() { Patch p{}; check(zh_porta_patch_default(&p), "zh_porta_patch_default"); return p; }
    void getState(State *host) const { check(zh_porta_get_state(h_, host), "zh_porta_get_state"); }
    void setState(const State *host) { check(zh_porta_set_state(h_, host), "zh_porta_set_state"); }
    void paint(Span span, const std::array<zh_buf, 2> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_porta_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_porta_paint");
    }
    // MainModule's Trigger loop (:119-128) for every voice in one call; span_params = host array [ZH_PORTA_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 2> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_porta_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_porta_paint_spans");
    }
};

// Instrument of examples/example_vibrato.zig (:17-69) for n voices as one fused kernel: a pulse whose frequency a slow sine
// modulates, times a gate.  Outputs as Porta's
class Vibrato {
    zh_vibrato *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 2;
    static constexpr size_t num_temps = 3;
    using Params = zh_vibrato_params;
    using Patch = zh_vibrato_patch;
    using State = zh_vibrato_state;
    Vibrato(Context &ctx, uint32_t n_voices) { check(zh_vibrato_create(ctx.get(), n_voices, &h_), "zh_vibrato_create"); }
    ~Vibrato() { if (h_) zh_vibrato_destroy(h_); }
    Vibrato(const Vibrato &) = delete;
    Vibrato &operator=(const Vibrato &) = delete;
    zh_vibrato *get() const { return h_; }
    static Patch defaultPatch() { Patch p{}; check(zh_vibrato_patch_default(&p), "zh_vibrato_patch_default"); return p; }
    void getState(State *host) const { check(zh_vibrato_get_state(h_, host), "zh_vibrato_get_state"); }
    void setState(const State *host) { check(zh_vibrato_set_state(h_, host), "zh_vibrato_set_state"); }
    void paint(Span span, const std::array<zh_buf, 2> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_vibrato_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_vibrato_paint");
    }
    // MainModule's Trigger loop (:101-110) for every voice in one call; span_params = host array [ZH_VIBRATO_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 2> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_vibrato_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_vibrato_paint_spans");
    }
};

// HardSquareInstrument of examples/modules.zig (:250-289) for n voices as one fused kernel: a pulse of color 0.5 times a gate, with
// the frequency image examples/example_arpeggiator.zig:115 adds beside it.  Outputs as Porta's
class HardSquare {
    zh_hard_square *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 2;
    static constexpr size_t num_temps = 2;
    using Params = zh_hard_square_params;
    using State = zh_hard_square_state;
    HardSquare(Context &ctx, uint32_t n_voices) { check(zh_hard_square_create(ctx.get(), n_voices, &h_), "zh_hard_square_create"); }
    ~HardSquare() { if (h_) zh_hard_square_destroy(h_); }
    HardSquare(const HardSquare &) = delete;
    HardSquare &operator=(const HardSquare &) = delete;
    zh_hard_square *get() const { return h_; }
    void getState(State *host) const { check(zh_hard_square_get_state(h_, host), "zh_hard_square_get_state"); }
    void setState(const State *host) { check(zh_hard_square_set_state(h_, host), "zh_hard_square_set_state"); }
    void paint(Span span, const std::array<zh_buf, 2> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_hard_square_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_hard_square_paint");
    }
    // Arpeggiator.paint's Trigger loop (:106-116) for every voice in one call; span_params = host array [ZH_HARD_SQUARE_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 2> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_hard_square_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_hard_square_paint_spans");
    }
};

// What the stage classes below (Arp, Subsong, SpanMerge) share: the handle and the table side of zh_<stage>_*, by its C functions.
// `prefix` ("zh_arp") is what an Error names
template <class H, int (*Destroy)(H *), int (*Reserve)(H *, uint32_t), int (*ScriptTable)(const H *, uint32_t, zh_script_span_table *),
          int (*SpanParam)(const H *, uint32_t, zh_script_span_param *), int (*Overflows)(H *, uint64_t *)>
class Stage {
protected:
    H *h_ = nullptr;
    const char *prefix_;
    explicit Stage(const char *prefix) : prefix_(prefix) {}
    ~Stage() { if (h_) Destroy(h_); }
    void checked(int rc, const char *fn) const { if (rc != 0) throw Error(rc, std::string(prefix_) + fn); }

public:
    Stage(const Stage &) = delete;
    Stage &operator=(const Stage &) = delete;
    H *get() const { return h_; }
    void reserve(uint32_t max_rows) { checked(Reserve(h_, max_rows), "_reserve"); }               // invalidates views and graphs
    zh_script_span_table scriptTable(uint32_t max_spans) const {
        zh_script_span_table t{};
        checked(ScriptTable(h_, max_spans, &t), "_script_table");
        return t;
    }
    zh_script_span_param spanParam(uint32_t field) const {
        zh_script_span_param p{};
        checked(SpanParam(h_, field, &p), "_span_param");
        return p;
    }
    uint64_t overflows() { uint64_t n = 0; checked(Overflows(h_, &n), "_overflows"); return n; }
};

// Arpeggiator.paint of examples/example_arpeggiator.zig (:49-107) without its instrument, for n players on the device: a stage
// between a live voice bank of polyphony 1 (records {held_lo, held_hi, on = 1}) and a voice's paintSpans
class Arp : public Stage<zh_arp, zh_arp_destroy, zh_arp_reserve, zh_arp_script_table, zh_arp_span_param, zh_arp_overflows> {
public:
    using State = zh_arp_state;
    Arp(Context &ctx, uint32_t n_players, const float *key_freqs, uint32_t n_keys) : Stage("zh_arp") {
        check(zh_arp_create(ctx.get(), n_players, key_freqs, n_keys, &h_), "zh_arp_create");
    }
    void reset() { check(zh_arp_reset(h_), "zh_arp_reset"); }                                     // init() :38-47
    // one buffer: `in` and held[2] are the outer bank's views (zh_voice_bank_script_table, zh_voice_bank_span_param of words 0 and 1)
    void schedule(float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table &in, const zh_script_span_param *held) {
        check(zh_arp_schedule(h_, sample_rate, out_len, max_spans, &in, held), "zh_arp_schedule");
    }
    void getState(State *host) const { check(zh_arp_get_state(h_, host), "zh_arp_get_state"); }
    void setState(const State *host) { check(zh_arp_set_state(h_, host), "zh_arp_set_state"); }
};

// Polyphony.paint of examples/example_polyphony.zig (:61-92) without its instruments, for n players of n_keys always-running voices
// on the device: a stage between a live voice bank of polyphony 1 (records {held_lo, held_hi, on = 1}) and a voice's span paint;
// voice = player * n_keys + key
class KeyFan : public Stage<zh_keyfan, zh_keyfan_destroy, zh_keyfan_reserve, zh_keyfan_script_table, zh_keyfan_span_param, zh_keyfan_overflows> {
public:
    using State = zh_keyfan_state;
    KeyFan(Context &ctx, uint32_t n_players, const float *key_freqs, uint32_t n_keys) : Stage("zh_keyfan") {
        check(zh_keyfan_create(ctx.get(), n_players, key_freqs, n_keys, &h_), "zh_keyfan_create");
    }
    void reset() { check(zh_keyfan_reset(h_), "zh_keyfan_reset"); }                               // Voice :50-56
    // one buffer: `in` and held[2] are the outer bank's views (zh_voice_bank_script_table, zh_voice_bank_span_param of words 0 and 1)
    void schedule(uint32_t out_len, uint32_t max_spans, const zh_script_span_table &in, const zh_script_span_param *held) {
        check(zh_keyfan_schedule(h_, out_len, max_spans, &in, held), "zh_keyfan_schedule");
    }
    // the view zh_nice_paint_spans and zh_pmosc_paint_spans take (paintSpans below)
    zh_span_table spanTable(uint32_t max_spans) const {
        zh_span_table t{};
        check(zh_keyfan_span_table(h_, max_spans, &t), "zh_keyfan_span_table");
        return t;
    }
    void getState(State *host) const { check(zh_keyfan_get_state(h_, host), "zh_keyfan_get_state"); }
    void setState(const State *host) { check(zh_keyfan_set_state(h_, host), "zh_keyfan_set_state"); }
};

// InnerInstrument of examples/example_subsong.zig (:24-68) for n voices as one fused kernel: a sawtooth of constant frequency
// times an envelope whose curves are cubed; one output
class SawEnv {
    zh_saw_env *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 1;
    static constexpr size_t num_temps = 2;
    using Params = zh_saw_env_params;
    using Patch = zh_saw_env_patch;
    using State = zh_saw_env_state;
    SawEnv(Context &ctx, uint32_t n_voices) { check(zh_saw_env_create(ctx.get(), n_voices, &h_), "zh_saw_env_create"); }
    ~SawEnv() { if (h_) zh_saw_env_destroy(h_); }
    SawEnv(const SawEnv &) = delete;
    SawEnv &operator=(const SawEnv &) = delete;
    zh_saw_env *get() const { return h_; }
    static Patch defaultPatch() { Patch p{}; check(zh_saw_env_patch_default(&p), "zh_saw_env_patch_default"); return p; }
    void getState(State *host) const { check(zh_saw_env_get_state(h_, host), "zh_saw_env_get_state"); }
    void setState(const State *host) { check(zh_saw_env_set_state(h_, host), "zh_saw_env_set_state"); }
    void paint(Span span, const std::array<zh_buf, 1> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_saw_env_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_saw_env_paint");
    }
    // SubtrackPlayer.paint's Trigger loop (:135-143) for every voice in one call; span_params = host array [ZH_SAW_ENV_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 1> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_saw_env_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_saw_env_paint_spans");
    }
};

// K canned songs (src/zang/notes.zig:130-134) on the device: melody m = events [offsets[m], offsets[m + 1]); immutable
class MelodyKit {
    zh_melody_kit *h_ = nullptr;

public:
    using Event = zh_melody_event;
    MelodyKit(Context &ctx, const uint32_t *offsets, uint32_t n_melodies, const Event *events, uint32_t n_events) {
        check(zh_melody_kit_create(ctx.get(), offsets, n_melodies, events, n_events, &h_), "zh_melody_kit_create");
    }
    ~MelodyKit() { if (h_) zh_melody_kit_destroy(h_); }
    MelodyKit(const MelodyKit &) = delete;
    MelodyKit &operator=(const MelodyKit &) = delete;
    zh_melody_kit *get() const { return h_; }
    uint32_t count() const { uint32_t k = 0; check(zh_melody_kit_count(h_, &k, nullptr), "zh_melody_kit_count"); return k; }
};

// SubtrackPlayer.paint of examples/example_subsong.zig (:122-144) without its instrument, for n players on the device: a stage
// between a live voice bank of polyphony 1 (records {freq, note_on, melody}) and a voice's paintSpans.  The kit outlives the stage
class Subsong : public Stage<zh_subsong, zh_subsong_destroy, zh_subsong_reserve, zh_subsong_script_table, zh_subsong_span_param, zh_subsong_overflows> {
public:
    using State = zh_subsong_state;
    Subsong(Context &ctx, uint32_t n_players, const MelodyKit &kit, float base_freq) : Stage("zh_subsong") {
        check(zh_subsong_create(ctx.get(), n_players, kit.get(), base_freq, &h_), "zh_subsong_create");
    }
    void reset() { check(zh_subsong_reset(h_), "zh_subsong_reset"); }                             // init() :104-120
    // one buffer: `in` and outer[ZH_SUBSONG_IN_FIELDS] are the outer bank's views (zh_voice_bank_script_table, zh_voice_bank_span_param)
    void schedule(float sample_rate, uint32_t out_len, uint32_t max_spans, const zh_script_span_table &in, const zh_script_span_param *outer) {
        check(zh_subsong_schedule(h_, sample_rate, out_len, max_spans, &in, outer), "zh_subsong_schedule");
    }
    void getState(State *host) const { check(zh_subsong_get_state(h_, host), "zh_subsong_get_state"); }
    void setState(const State *host) { check(zh_subsong_set_state(h_, host), "zh_subsong_set_state"); }
};

// The loop of examples/example_two.zig (:93-151) without its voice, for n players on the device: two span tables (two live voice
// banks of polyphony 1, say) merged into one, which a voice's paintSpans reads in place.  Stateless
class SpanMerge : public Stage<zh_span_merge, zh_span_merge_destroy, zh_span_merge_reserve, zh_span_merge_script_table, zh_span_merge_span_param,
                               zh_span_merge_overflows> {
    uint32_t own_ = 0;

public:
    using Source = zh_span_merge_source;
    SpanMerge(Context &ctx, uint32_t n_players, const Source &a, const Source &b) : Stage("zh_span_merge"), own_(a.n_fields + b.n_fields) {
        check(zh_span_merge_create(ctx.get(), n_players, &a, &b, &h_), "zh_span_merge_create");
    }
    // one buffer: each source's table and its field arrays [n_fields]
    void schedule(uint32_t out_len, uint32_t max_spans, const zh_script_span_table &in_a, const zh_script_span_param *fields_a,
                  const zh_script_span_table &in_b, const zh_script_span_param *fields_b) {
        check(zh_span_merge_schedule(h_, out_len, max_spans, &in_a, fields_a, &in_b, fields_b), "zh_span_merge_schedule");
    }
    // spanParam's field: A's, then B's, then ownField(ZH_SPAN_MERGE_NOTE_ON / _NIC_A / _NIC_B)
    uint32_t ownField(uint32_t which) const { return own_ + which; }
};

// What one inner span of examples/example_two.zig (:109-138, :153) does, for n voices as one fused kernel: a TriSawOsc of constant
// frequency and color times an envelope whose curves are cubed, with the frequency image beside it.  Outputs as Porta's
class Dual {
    zh_dual *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 2;
    static constexpr size_t num_temps = 2;
    using Params = zh_dual_params;
    using Patch = zh_dual_patch;
    using State = zh_dual_state;
    Dual(Context &ctx, uint32_t n_voices) { check(zh_dual_create(ctx.get(), n_voices, &h_), "zh_dual_create"); }
    ~Dual() { if (h_) zh_dual_destroy(h_); }
    Dual(const Dual &) = delete;
    Dual &operator=(const Dual &) = delete;
    zh_dual *get() const { return h_; }
    static Patch defaultPatch() { Patch p{}; check(zh_dual_patch_default(&p), "zh_dual_patch_default"); return p; }
    void getState(State *host) const { check(zh_dual_get_state(h_, host), "zh_dual_get_state"); }
    void setState(const State *host) { check(zh_dual_set_state(h_, host), "zh_dual_set_state"); }
    void paint(Span span, const std::array<zh_buf, 2> &outputs, zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_dual_paint(h_, span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_dual_paint");
    }
    // the merge loop (:101-151) for every voice in one call; span_params = host array [ZH_DUAL_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 2> &outputs, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_dual_paint_spans(h_, span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags), "zh_dual_paint_spans");
    }
};

// The PMOscInstrument of examples/example_mouse.zig (:24-73) for n voices as one fused kernel: `relative` is a parameter, ratio and
// multiplier are zh_cob signals.  temps: nullptr, or three zh_buf of which [1] may be the carried image of the reference's stale temp
// (zang_hip.h, "ONE DIFFERENCE").  paintControlled is MainModule.paint (:148-211): each control a Portamento over its own table.
class PMCtl {
    zh_pmctl *h_ = nullptr;

public:
    static constexpr size_t num_outputs = 1;
    static constexpr size_t num_temps = 3;
    using Params = zh_pmctl_params;
    using Patch = zh_pmctl_patch;
    using State = zh_pmctl_state;
    using Control = zh_pmctl_control;
    PMCtl(Context &ctx, uint32_t n_voices) { check(zh_pmctl_create(ctx.get(), n_voices, &h_), "zh_pmctl_create"); }
    ~PMCtl() { if (h_) zh_pmctl_destroy(h_); }
    PMCtl(const PMCtl &) = delete;
    PMCtl &operator=(const PMCtl &) = delete;
    zh_pmctl *get() const { return h_; }
    static Patch defaultPatch() { Patch p{}; check(zh_pmctl_patch_default(&p), "zh_pmctl_patch_default"); return p; }
    void getState(State *host) const { check(zh_pmctl_get_state(h_, host), "zh_pmctl_get_state"); }
    void setState(const State *host) { check(zh_pmctl_set_state(h_, host), "zh_pmctl_set_state"); }
    void paint(Span span, const std::array<zh_buf, 1> &outputs, const zh_buf *temps, zh_bool note_id_changed, const Params &params,
               const zh_cob &ratio, const zh_cob &multiplier, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_pmctl_paint(h_, span.start, span.end, outputs.data(), temps, note_id_changed, &params, &ratio, &multiplier, flags), "zh_pmctl_paint");
    }
    // the Trigger loop (:193-211) for every voice in one call; span_params = host array [ZH_PMCTL_SPAN_FIELDS] or nullptr
    void paintSpans(Span span, const std::array<zh_buf, 1> &outputs, const zh_buf *temps, const Params &params, const zh_script_span_param *span_params,
                    const zh_script_span_table &table, const zh_cob &ratio, const zh_cob &multiplier, uint32_t flags = ZH_PAINT_ADD) {
        check(zh_pmctl_paint_spans(h_, span.start, span.end, outputs.data(), temps, &params, span_params, &table, &ratio, &multiplier, flags),
              "zh_pmctl_paint_spans");
    }
    void paintControlled(Span span, const std::array<zh_buf, 1> &outputs, const zh_buf *temps, const Params &params,
                         const zh_script_span_param *span_params, const zh_script_span_table &notes, const Control &ratio, const Control &multiplier,
                         uint32_t flags = ZH_PAINT_ADD) {
        check(zh_pmctl_paint_controlled(h_, span.start, span.end, outputs.data(), temps, &params, span_params, &notes, &ratio, &multiplier, flags),
              "zh_pmctl_paint_controlled");
    }
};

}  // namespace zang

namespace mod {

// One class per module: `num_outputs`, `num_temps`, `Params` (the C ABI's params struct, fields in the Zig
// declaration order) and paint(span, outputs, temps, note_id_changed, params) like the Zig declarations.
// SPANS: ZANG_HIP_SPANS(prefix) adds paint_spans(span, outputs, temps, params, span_params, table) -- zh_<prefix>_paint_spans: the
// reference's Trigger loop (one paint per sub-span of a per-voice table) for every voice in one call
#define ZANG_HIP_MODULE(Name, prefix, NT, CREATE_ARGS_DECL, CREATE_ARGS_USE, SPANS)                                     \
    class Name {                                                                                                          \
        zh_##prefix *h_ = nullptr;                                                                                        \
                                                                                                                          \
    public:                                                                                                               \
        static constexpr size_t num_outputs = 1;                                                                          \
        static constexpr size_t num_temps = NT;                                                                           \
        using Params = zh_##prefix##_params;                                                                              \
        Name(zang::Context &ctx, uint32_t n_voices CREATE_ARGS_DECL) {                                                    \
            zang::check(zh_##prefix##_create(ctx.get(), n_voices CREATE_ARGS_USE, &h_), "zh_" #prefix "_create");         \
        }                                                                                                                 \
        ~Name() { if (h_) zh_##prefix##_destroy(h_); }                                                                    \
        Name(const Name &) = delete;                                                                                      \
        Name &operator=(const Name &) = delete;                                                                           \
        zh_##prefix *get() const { return h_; }                                                                           \
        void paint(zang::Span span, const std::array<zh_buf, 1> &outputs, const std::array<zh_buf, NT> &temps,            \
                   zh_bool note_id_changed, const Params &params, uint32_t flags = ZH_PAINT_ADD) {                        \
            zang::check(zh_##prefix##_paint(h_, span.start, span.end, outputs.data(), NT ? temps.data() : nullptr,         \
                                            note_id_changed, &params, flags), "zh_" #prefix "_paint");                     \
        }                                                                                                                 \
        SPANS                                                                                                             \
    };
#define ZANG_HIP_SPANS(prefix)                                                                                            \
    void paint_spans(zang::Span span, const std::array<zh_buf, 1> &outputs, const std::array<zh_buf, num_temps> &temps,   \
                     const Params &params, const zh_script_span_param *span_params, const zh_script_span_table &table,  \
                     uint32_t flags = ZH_PAINT_ADD) {                                                                     \
        zang::check(zh_##prefix##_paint_spans(h_, span.start, span.end, outputs.data(), num_temps ? temps.data() : nullptr,  \
                                              &params, span_params, &table, flags), "zh_" #prefix "_paint_spans");       \
    }

#define ZANG_HIP_NO_ARGS
#define ZANG_HIP_COMMA_SEED , uint64_t first_seed = 0
#define ZANG_HIP_USE_SEED , first_seed
#define ZANG_HIP_COMMA_F32 , zh_f32 init_value
#define ZANG_HIP_USE_F32 , init_value

ZANG_HIP_MODULE(SineOsc, sineosc, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(sineosc))            // src/modules/SineOsc.zig
ZANG_HIP_MODULE(PulseOsc, pulseosc, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(pulseosc))          // src/modules/PulseOsc.zig
ZANG_HIP_MODULE(TriSawOsc, trisawosc, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(trisawosc))        // src/modules/TriSawOsc.zig
ZANG_HIP_MODULE(Noise, noise, 0, ZANG_HIP_COMMA_SEED, ZANG_HIP_USE_SEED, ZANG_HIP_SPANS(noise))            // src/modules/Noise.zig (seed = first_seed + voice)
ZANG_HIP_MODULE(Envelope, envelope, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(envelope))          // src/modules/Envelope.zig
ZANG_HIP_MODULE(Gate, gate, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(gate))                  // src/modules/Gate.zig
ZANG_HIP_MODULE(Filter, filter, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(filter))              // src/modules/Filter.zig
ZANG_HIP_MODULE(Sampler, sampler, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(sampler))     // src/modules/Sampler.zig
ZANG_HIP_MODULE(Decimator, decimator, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(decimator))        // src/modules/Decimator.zig
ZANG_HIP_MODULE(Distortion, distortion, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_SPANS(distortion))      // src/modules/Distortion.zig
ZANG_HIP_MODULE(Cycle, cycle, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS)                // src/modules/Cycle.zig
ZANG_HIP_MODULE(Portamento, portamento, 0, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS, ZANG_HIP_NO_ARGS)      // src/modules/Portamento.zig
// the fused composites of examples/modules.zig (temps are accepted and unused: they live in registers)
ZANG_HIP_MODULE(NiceInstrument, nice, 2, ZANG_HIP_COMMA_F32, ZANG_HIP_USE_F32, ZANG_HIP_NO_ARGS)      // :189-248, init(color)
ZANG_HIP_MODULE(PMOscInstrument, pmosc, 3, ZANG_HIP_COMMA_F32, ZANG_HIP_USE_F32, ZANG_HIP_NO_ARGS)    // :80-128, init(release_duration)

#undef ZANG_HIP_MODULE
#undef ZANG_HIP_SPANS
#undef ZANG_HIP_NO_ARGS
#undef ZANG_HIP_COMMA_SEED
#undef ZANG_HIP_USE_SEED
#undef ZANG_HIP_COMMA_F32
#undef ZANG_HIP_USE_F32

// The decimated group mix (examples/example_polyphony.zig:135-163 for every group): `m` has one voice per group of `src`; group g's
// voices are added in order from +0 and go through its Decimator -- or straight on, modes_dev[g].bypass -- onto row g of dst_dev
inline void paintGroups(Decimator &m, zang::Span span, float *dst_dev, size_t dst_stride_floats, zh_buf src, uint32_t group_voices,
                        float sample_rate, const zh_group_decimation *modes_dev, uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_decimator_paint_groups(m.get(), span.start, span.end, dst_dev, dst_stride_floats, src, group_voices, sample_rate, modes_dev, flags),
                "zh_decimator_paint_groups");
}

// The Sampler over a sample kit: the sample and the channel are per-voice / per-note values like the rate and the loop flag
// (Sampler.zig:62-67).  paintKit: n Samplers, each with its own sample, over one span; paintKitSpans: the Trigger loop, span_params
// = host array [ZH_SAMPLER_KIT_SPAN_FIELDS] or nullptr.
inline void paintKit(Sampler &m, zang::Span span, const std::array<zh_buf, 1> &outputs, zh_bool note_id_changed, const zh_sampler_kit_params &params,
                     uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_sampler_paint_kit(m.get(), span.start, span.end, outputs.data(), nullptr, note_id_changed, &params, flags), "zh_sampler_paint_kit");
}
inline void paintKitSpans(Sampler &m, zang::Span span, const std::array<zh_buf, 1> &outputs, const zh_sampler_kit_params &params,
                          const zh_script_span_param *span_params, const zh_script_span_table &table, uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_sampler_paint_kit_spans(m.get(), span.start, span.end, outputs.data(), nullptr, &params, span_params, &table, flags),
                "zh_sampler_paint_kit_spans");
}

// NiceInstrument painted and mixed down over its voices without materialising per-voice output: mono, or two channels with a
// per-voice gain each (a two-output module fed `voice * pan_c`, examples/example_stereo.zig:92-98)
inline void paintMix(NiceInstrument &m, zang::Span span, float *mix_dev, zh_bool note_id_changed, const NiceInstrument::Params &params,
                     uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_nice_paint_mix(m.get(), span.start, span.end, mix_dev, note_id_changed, &params, flags), "zh_nice_paint_mix");
}
inline void paintMixStereo(NiceInstrument &m, zang::Span span, float *mix_left_dev, float *mix_right_dev, zh_f32 gain_left, zh_f32 gain_right,
                           zh_bool note_id_changed, const NiceInstrument::Params &params, uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_nice_paint_mix_stereo(m.get(), span.start, span.end, mix_left_dev, mix_right_dev, gain_left, gain_right, note_id_changed,
                                         &params, flags), "zh_nice_paint_mix_stereo");
}
// n consecutive paintMixStereo calls (per-buffer params and note_id_changed) as one launch: state in registers between buffers
inline void paintMixStereoBatch(NiceInstrument &m, zang::Span span, const std::vector<float *> &mix_left_dev, const std::vector<float *> &mix_right_dev,
                                zh_f32 gain_left, zh_f32 gain_right, const std::vector<zh_bool> &note_id_changed,
                                const std::vector<NiceInstrument::Params> &params, uint32_t flags = ZH_PAINT_ADD) {
    if (mix_left_dev.size() != params.size() || mix_right_dev.size() != params.size() || note_id_changed.size() != params.size())
        throw zang::Error(ZH_ERR_INVALID, "paintMixStereoBatch: one mix pair, one note_id_changed and one Params per buffer");
    zang::check(zh_nice_paint_mix_stereo_batch(m.get(), span.start, span.end, (uint32_t)params.size(), mix_left_dev.data(), mix_right_dev.data(),
                                               gain_left, gain_right, note_id_changed.data(), params.data(), flags), "zh_nice_paint_mix_stereo_batch");
}
// n consecutive paints of a constant-frequency oscillator (same span and params, buffer b into outputs[b]) as one launch
inline void paintBatch(PulseOsc &m, zang::Span span, const std::vector<zh_buf> &outputs, const PulseOsc::Params &params, uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_pulseosc_paint_batch(m.get(), span.start, span.end, outputs.data(), (uint32_t)outputs.size(), &params, flags), "zh_pulseosc_paint_batch");
}
inline void paintBatch(TriSawOsc &m, zang::Span span, const std::vector<zh_buf> &outputs, const TriSawOsc::Params &params, uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_trisawosc_paint_batch(m.get(), span.start, span.end, outputs.data(), (uint32_t)outputs.size(), &params, flags), "zh_trisawosc_paint_batch");
}

// the fused composites over a per-voice sub-span table (zh_span_table: uploaded by the host, or a zang::VoiceBank's spanTable())
inline void paintSpans(NiceInstrument &m, zang::Span span, const std::array<zh_buf, 1> &outputs, float sample_rate, const zh_span_table &table,
                       uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_nice_paint_spans(m.get(), span.start, span.end, outputs.data(), nullptr, sample_rate, &table, flags), "zh_nice_paint_spans");
}
inline void paintSpans(PMOscInstrument &m, zang::Span span, const std::array<zh_buf, 1> &outputs, float sample_rate, const zh_span_table &table,
                       uint32_t flags = ZH_PAINT_ADD) {
    zang::check(zh_pmosc_paint_spans(m.get(), span.start, span.end, outputs.data(), nullptr, sample_rate, &table, flags), "zh_pmosc_paint_spans");
}

// mod.Filter.cutoffFromFrequency (Filter.zig:20-23), elementwise on the device
inline void cutoffFromFrequency(zang::Context &c, uint32_t n, float *cutoff_out_dev, const float *frequency_dev, float sample_rate) {
    zang::check(zh_filter_cutoff_from_frequency(c.get(), n, cutoff_out_dev, frequency_dev, sample_rate), "cutoffFromFrequency");
}

}  // namespace mod

// std.math.sin / cos / pow (f32) elementwise on the device, bit-identical to what the modules compute with
namespace zang { namespace math {
inline void sin(zang::Context &c, uint32_t n, float *out_dev, const float *x_dev) { zang::check(zh_sin(c.get(), n, out_dev, x_dev), "sin"); }
inline void cos(zang::Context &c, uint32_t n, float *out_dev, const float *x_dev) { zang::check(zh_cos(c.get(), n, out_dev, x_dev), "cos"); }
inline void atan(zang::Context &c, uint32_t n, float *out_dev, const float *x_dev) { zang::check(zh_atan(c.get(), n, out_dev, x_dev), "atan"); }
inline void pow(zang::Context &c, uint32_t n, float *out_dev, const float *x_dev, const float *y_dev) { zang::check(zh_pow(c.get(), n, out_dev, x_dev, y_dev), "pow"); }
} }  // namespace zang::math
