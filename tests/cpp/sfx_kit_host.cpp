// sfx_kit_host.cpp -- the effect kit's packing (zang_amd/csrc/laser.hip.h lk_describe / lk_pack: what zh_sfx_kit_create runs) as a
// stand-alone program for AddressSanitizer + UBSan.  Three kits -- empty curves only, one effect, five effects of unequal lengths
// -- each packed into a heap block of EXACTLY the size the library allocates, then every descriptor and node read back and
// compared; what the library refuses is refused here.
#include <cstdio>
#include <vector>

#include "../../zang_amd/csrc/laser.hip.h"

static int fail(const char *what, int a = 0, int b = 0) { printf("%s (%d, %d)\nFAIL\n", what, a, b); return 1; }

static int run(const std::vector<std::vector<zh_curve_node>> &curves, const std::vector<uint32_t> &fn) {
    const uint32_t n = (uint32_t)(curves.size() / 3);
    std::vector<zh_sfx_effect> effects(n);
    for (uint32_t i = 0; i < n; i++) {
        zh_sfx_curve c[3];
        for (int k = 0; k < 3; k++) {
            const std::vector<zh_curve_node> &v = curves[3 * i + k];
            c[k] = zh_sfx_curve{v.empty() ? nullptr : v.data(), (uint32_t)v.size(), fn[3 * i + k]};
        }
        effects[i] = zh_sfx_effect{c[0], c[1], c[2]};
    }
    LkEffectDesc *desc = new LkEffectDesc[n];
    size_t count = 0;
    if (lk_describe(effects.data(), n, desc, &count) != ZH_OK) { delete[] desc; return fail("describe"); }
    size_t total = 0, longest = 0;
    for (const auto &v : curves) { total += v.size(); longest = v.size() > longest ? v.size() : longest; }
    if (count != total + longest) { delete[] desc; return fail("array length", (int)count, (int)(total + longest)); }
    zh_curve_node *array = new zh_curve_node[count];                              // exactly the library's size
    lk_pack(effects.data(), n, desc, array, count);
    int rc = 0;
    size_t at = 0;
    for (uint32_t i = 0; i < n && !rc; i++)
        for (int k = 0; k < 3 && !rc; k++) {
            const std::vector<zh_curve_node> &v = curves[3 * i + k];
            const LkCurveDesc d = desc[i].curve[k];
            if (d.offset != at || d.count != v.size() || d.function != fn[3 * i + k]) rc = fail("descriptor", (int)i, k);
            for (size_t j = 0; j < v.size() && !rc; j++)
                if (array[d.offset + j].value != v[j].value || array[d.offset + j].t != v[j].t) rc = fail("node", (int)i, (int)j);
            at += v.size();
        }
    for (size_t j = total; j < count && !rc; j++)                                   // the tail: the longest curve's length in zero nodes
        if (array[j].value != 0.0f || array[j].t != 0.0f) rc = fail("tail", (int)j);
    // the last index a carried node can have, from the last curve's first node
    if (!rc && n && count) { const LkCurveDesc d = desc[n - 1].curve[LK_VOLUME]; if (longest && d.offset + longest - 1 >= count) rc = fail("tail reach"); }
    delete[] array;
    delete[] desc;
    return rc;
}

static std::vector<zh_curve_node> curve(size_t n, float seed) {
    std::vector<zh_curve_node> v(n);
    for (size_t j = 0; j < n; j++) v[j] = zh_curve_node{seed + (float)j * 0.5f, (float)j * 0.001f};
    return v;
}

int main() {
    // empty curves only: an array of no nodes at all
    if (run({{}, {}, {}}, {0, 1, 0})) return 1;
    // one effect
    if (run({curve(3, 1.0f), curve(3, 2.0f), curve(3, 3.0f)}, {1, 1, 1})) return 1;
    // five effects of unequal lengths, the longest curve first and an empty one last
    std::vector<std::vector<zh_curve_node>> c;
    std::vector<uint32_t> fn;
    const size_t lens[15] = {40, 3, 3, 1, 0, 2, 7, 7, 7, 33, 1, 5, 2, 35, 0};
    for (int j = 0; j < 15; j++) { c.push_back(curve(lens[j], (float)j)); fn.push_back((uint32_t)(j % 2)); }
    if (run(c, fn)) return 1;
    // refusals: no effects, a NULL list with a count, a function outside the enum
    LkEffectDesc d[1];
    size_t count = 0;
    zh_sfx_effect e{};
    if (lk_describe(&e, 0, d, &count) != ZH_ERR_INVALID || lk_describe(nullptr, 1, d, &count) != ZH_ERR_INVALID) return fail("n == 0 accepted");
    e.carrier.count = 2;
    if (lk_describe(&e, 1, d, &count) != ZH_ERR_INVALID) return fail("NULL nodes accepted");
    e.carrier.count = 0; e.volume.function = 2;
    if (lk_describe(&e, 1, d, &count) != ZH_ERR_INVALID) return fail("function 2 accepted");
    e.volume.function = 1;
    if (lk_describe(&e, 1, d, &count) != ZH_OK || count != 0) return fail("an effect of empty curves refused");
    printf("PASS\n");
    return 0;
}
