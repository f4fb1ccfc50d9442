// state_block.hip.h -- the host side of every module whose state is one uint32_t[kWords][n] device block.  Three parts:
//   the float <-> word pair and VoiceLayout, what a Layout is made of, as plain C++ (the stand-alone harnesses of tests/cpp include
//   it through the headers that declare the Layouts: module_state.hip.h, fm.hip.h, lead.hip.h, ...);
//   the block level (hipcc only): the one pair of upload / download helpers, allocate-and-zero, and block_get_state /
//   block_set_state, a block <-> the ABI's array of structs over a Layout;
//   the flipper level: zh_flipper's (common.hip.h) two blocks -- flip_alloc / flip_free for a module that allocates more beside
//   them, flip_create / flip_destroy for one that does not, flip_get_state / flip_set_state over the CURRENT block.
// The single-block voice handles (zh_voice: create / destroy / get_state / set_state) and everything about painting: span_voice.hip.h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/zang_hip.h"

inline uint32_t zh_f32_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
inline float zh_bits_f32(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// A Layout is what the host side reads of a module's state, plain C++ beside the module's struct or lane:
//   State                                   the ABI struct of one voice
//   kWords                                  words per voice; the device block is uint32_t[kWords][n]
//   pack(s, w, n, v) / unpack(s, w, n, v)   voice v of n: struct -> rows and back
// (tests/cpp/lead_state_host.cpp and module_state_host.cpp run them under ASan and UBSan.)
template <class S, int WORDS, void (*PACK)(const S &, uint32_t *, size_t, size_t), void (*UNPACK)(S &, const uint32_t *, size_t, size_t)>
struct VoiceLayout {
    using State = S;
    enum { kWords = WORDS };
    static void pack(const State &s, uint32_t *w, size_t n, size_t v) { PACK(s, w, n, v); }
    static void unpack(State &s, const uint32_t *w, size_t n, size_t v) { UNPACK(s, w, n, v); }
};

#if defined(__HIPCC__)
#include "common.hip.h"
#include <new>
#include <vector>

// ---- the block level ---------------------------------------------------------------------------------------------------
template <typename T> static int upload_field(zh_ctx *ctx, T *dev, const std::vector<T> &h) {
    return zh_upload(ctx, dev, h.data(), h.size() * sizeof(T));
}
template <typename T> static int download_field(zh_ctx *ctx, std::vector<T> &h, const T *dev, size_t n) {
    h.resize(n);
    return zh_download(ctx, h.data(), dev, n * sizeof(T));
}
// `count` words, zeroed on the context's stream.  On an error *p is what was allocated (or nullptr): the caller frees it.
static inline int dev_alloc_zeroed(zh_ctx *ctx, uint32_t **p, size_t count) {
    int rc = dev_alloc(p, count);
    if (!rc && count) { hipError_t e = hipMemsetAsync(*p, 0, count * 4, ctx->stream); if (e != hipSuccess) rc = (int)e; }
    return rc;
}
// block[LY::kWords][n] <-> host[n]; n = 0 moves nothing and is ZH_OK
template <class LY> static int block_get_state(zh_ctx *ctx, const uint32_t *block, size_t n, typename LY::State *host) {
    std::vector<uint32_t> w;
    int rc = download_field(ctx, w, block, (size_t)LY::kWords * n);
    if (rc) return rc;
    for (size_t v = 0; v < n; v++) LY::unpack(host[v], w.data(), n, v);
    return ZH_OK;
}
template <class LY> static int block_set_state(zh_ctx *ctx, uint32_t *block, size_t n, const typename LY::State *host) {
    std::vector<uint32_t> w((size_t)LY::kWords * n);
    for (size_t v = 0; v < n; v++) LY::pack(host[v], w.data(), n, v);
    return upload_field(ctx, block, w);
}

// ---- the flipper level -------------------------------------------------------------------------------------------------
// both blocks of `words` x n, zeroed; on an error flip_free(m) frees what there is
static inline int flip_alloc(zh_ctx *ctx, zh_flipper *m, uint32_t n, uint32_t words) {
    m->id = 0; m->ctx = ctx; m->n = n; m->cur = 0; m->words = words;
    m->cnt[0] = m->cnt[1] = nullptr;
    int rc = dev_alloc_zeroed(ctx, &m->cnt[0], (size_t)words * n);
    if (!rc) rc = dev_alloc_zeroed(ctx, &m->cnt[1], (size_t)words * n);
    return rc;
}
static inline void flip_free(zh_flipper *m) { (void)hipFree(m->cnt[0]); (void)hipFree(m->cnt[1]); }

// A module that is its two blocks and nothing else.  init(): every word zero, or `init` (one voice's state) in every voice
// of both blocks.
template <class LY, class M> static int flip_create(zh_ctx *ctx, uint32_t n, M **out, const typename LY::State *init = nullptr) {
    if (!ctx || !out) return ZH_ERR_INVALID;
    M *m = new (std::nothrow) M();
    if (!m) return ZH_ERR_INVALID;
    int rc = flip_alloc(ctx, m, n, LY::kWords);
    if (!rc && init) {
        const std::vector<typename LY::State> all(n, *init);
        for (int b = 0; b < 2 && !rc; b++) rc = block_set_state<LY>(ctx, m->cnt[b], n, all.data());
    }
    if (rc) { flip_free(m); delete m; return rc; }
    zh_flipper_register(m);
    *out = m;
    return ZH_OK;
}
template <class M> static int flip_destroy(M *m) {
    if (!m) return ZH_ERR_INVALID;
    (void)hipStreamSynchronize(m->ctx->stream);
    zh_flipper_unregister(m);
    flip_free(m);
    delete m;
    return ZH_OK;
}
// the block the next paint starts from (a graph launch may have flipped: ctx.hip keeps m->cur right)
template <class LY> static int flip_get_state(zh_flipper *m, typename LY::State *host) {
    if (!m || !host) return ZH_ERR_INVALID;
    return block_get_state<LY>(m->ctx, m->cnt[m->cur], m->n, host);
}
template <class LY> static int flip_set_state(zh_flipper *m, const typename LY::State *host) {
    if (!m || !host) return ZH_ERR_INVALID;
    return block_set_state<LY>(m->ctx, m->cnt[m->cur], m->n, host);
}
#endif   // __HIPCC__
