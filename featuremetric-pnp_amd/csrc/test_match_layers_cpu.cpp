// Stand-alone host program over fmpnp_exhaustive_match_layers_cpu (fmpnp_match_layers_cpu.cpp, with the assembly
// twin fmpnp_hypercolumn_cpu.cpp and the dense match's twin fmpnp_match_cpu.cpp linked in as the yardstick), for
// sanitizer runs of the twin outside Python: `make match-layers-sanitize` builds it with ASan + UBSan and runs it.
// Seeded layers and exactly-sized heap buffers (a read or write one element outside a layer, the descriptors or an
// output is an ASan report).  Per case: small-integer operands without normalisation against "assemble, then
// match" bit for bit (every intermediate is exact: equal sizes and dyadic resizes); real operands with and without
// normalisation against the same yardstick within a loose tolerance (the derived bound is the Python tests'); 1 and
// 3 threads and scores = NULL give the same bytes; padded descriptor rows and padded channel strides; every batch
// item; N = 0; the argument errors.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
double uni01() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

struct Shape {
    int C, H, W;
};

struct Case {
    const char *name;
    int B, H, W, N;
    std::vector<Shape> layers;
    int pad;     // extra elements per channel plane (stride_c = H_l * W_l + pad) and per descriptor row
    bool exact;  // the resizes are dyadic: integer operands give exact scores
};

int fail(const Case &c, const char *what, long long a, long long b) {
    printf("FAIL %s: %s (%lld, %lld)\n", c.name, what, a, b);
    return 1;
}

struct Out {
    std::vector<int> argmax;
    std::vector<float> top, kth, scores;
    std::vector<unsigned char> mask;
    explicit Out(int N, size_t WH = 0) : argmax((size_t)N), top((size_t)N), kth((size_t)N), scores((size_t)N * WH), mask((size_t)N) {}
    bool same(const Out &o) const {
        return !memcmp(argmax.data(), o.argmax.data(), 4 * argmax.size()) && !memcmp(top.data(), o.top.data(), 4 * top.size()) &&
               !memcmp(kth.data(), o.kth.data(), 4 * kth.size()) && !memcmp(mask.data(), o.mask.data(), mask.size());
    }
};

int run(const Case &c, bool ints, int flags) {
    const int L = (int)c.layers.size(), B = c.B, H = c.H, W = c.W, N = c.N, WH = H * W;
    std::vector<std::vector<float>> data((size_t)L);
    std::vector<fmpnp_hc_layer> ly((size_t)L);
    int C = 0;
    for (int l = 0; l < L; ++l) {
        const Shape &s = c.layers[(size_t)l];
        const long long sc = (long long)s.H * s.W + c.pad, sb = sc * s.C;
        data[(size_t)l].resize((size_t)(sb * B - c.pad));
        for (float &v : data[(size_t)l]) v = ints ? (float)((int)(uni01() * 5.0) - 2) : (float)(uni01() * 2.0 - 1.0);
        memset(&ly[(size_t)l], 0, sizeof ly[(size_t)l]);
        ly[(size_t)l].data = data[(size_t)l].data();
        ly[(size_t)l].C = s.C;
        ly[(size_t)l].H = s.H;
        ly[(size_t)l].W = s.W;
        ly[(size_t)l].stride_b = sb;
        ly[(size_t)l].stride_c = sc;
        ly[(size_t)l].stride_y = s.W;
        C += s.C;
    }
    const int ld = C + c.pad;
    std::vector<float> sparse((size_t)N * ld - c.pad);  // (the last row ends at its last channel)
    for (float &v : sparse) v = ints ? (float)((int)(uni01() * 5.0) - 2) : (float)(uni01() * 2.0 - 1.0);
    const int top_k = WH > 3 ? WH / 3 : 1;
    const double ratio = 0.9;

    std::vector<float> dense((size_t)B * C * WH);
    if (fmpnp_hypercolumn_assemble_cpu(ly.data(), L, B, dense.data(), H, W, (long long)C * WH, WH, W, flags, 2))
        return fail(c, "assembly twin", -1, -1);
    for (int item = 0; item < B; ++item) {
        Out want(N, (size_t)WH), got(N, (size_t)WH), quiet(N);
        if (fmpnp_exhaustive_match_cpu(sparse.data(), N, ld, dense.data() + (size_t)item * C * WH, C, WH, WH, top_k, ratio,
                                       want.argmax.data(), want.top.data(), want.kth.data(), want.mask.data(),
                                       want.scores.data(), 2))
            return fail(c, "dense twin", item, -1);
        for (int threads = 1; threads <= 3; threads += 2) {
            Out g(N, (size_t)WH);
            const int rc = fmpnp_exhaustive_match_layers_cpu(sparse.data(), N, ld, ly.data(), L, B, item, H, W, flags, top_k, ratio,
                                                             g.argmax.data(), g.top.data(), g.kth.data(), g.mask.data(),
                                                             g.scores.data(), threads);
            if (rc) return fail(c, "layered twin rc", rc, threads);
            if (threads == 1) got = g;
            else if (!g.same(got) || memcmp(g.scores.data(), got.scores.data(), 4 * g.scores.size()))
                return fail(c, "the thread count changes a row", item, threads);
        }
        if (fmpnp_exhaustive_match_layers_cpu(sparse.data(), N, ld, ly.data(), L, B, item, H, W, flags, top_k, ratio,
                                              quiet.argmax.data(), quiet.top.data(), quiet.kth.data(), quiet.mask.data(), nullptr, 2) ||
            !quiet.same(got))
            return fail(c, "scores = NULL changes a result", item, -1);
        if (ints && c.exact && !flags) {
            if (!got.same(want) || memcmp(got.scores.data(), want.scores.data(), 4 * got.scores.size()))
                return fail(c, "exact operands differ from assemble-then-match", item, -1);
        } else {
            for (int i = 0; i < N; ++i) {
                double l1 = 0.0;
                for (int k = 0; k < C; ++k) l1 += fabs((double)sparse[(size_t)i * ld + k]);
                const double tol = 1e-4 * (l1 + 1.0) * (flags ? 1.0 : 4.0);  // (|x| <= 1 normalised; <= 4 with integers)
                for (int p = 0; p < WH; ++p) {
                    const double a = got.scores[(size_t)i * WH + p], b = want.scores[(size_t)i * WH + p];
                    if (a != a && b != b) continue;  // (integers can make an all-zero texel: 0 / 0 in both)
                    if (!(fabs(a - b) <= tol)) return fail(c, "far from assemble-then-match", i, p);
                }
            }
        }
    }
    // N = 0 touches nothing (null buffers)
    if (fmpnp_exhaustive_match_layers_cpu(nullptr, 0, ld, ly.data(), L, B, 0, H, W, flags, top_k, ratio, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, 1))
        return fail(c, "N = 0", -1, -1);
    // argument errors
    Out o(N);
    auto call = [&](const fmpnp_hc_layer *layers, int L_, int item, int H_, int ld_, int flags_, int k, double r, int threads) {
        return fmpnp_exhaustive_match_layers_cpu(sparse.data(), N, ld_, layers, L_, B, item, H_, W, flags_, k, r, o.argmax.data(),
                                                 o.top.data(), o.kth.data(), o.mask.data(), nullptr, threads);
    };
    int bad = 0;
    bad += call(ly.data(), 0, 0, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), 9, 0, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(nullptr, L, 0, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, B, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, -1, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, 0, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, H, C - 1, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, H, ld, flags | FMPNP_HC_VECTOR_STORES, top_k, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, H, ld, flags, 0, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, H, ld, flags, WH + 1, ratio, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, H, ld, flags, top_k, NAN, 1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, H, ld, flags, top_k, ratio, -1) != FMPNP_EINVAL;
    bad += call(ly.data(), L, 0, (1 << 24) + 1, ld, flags, top_k, ratio, 1) != FMPNP_ETOOBIG;
    std::vector<fmpnp_hc_layer> bent = ly;
    bent[0].stride_y += 1;  // a padded row: the correlation cannot read the plane as [H_l * W_l]
    bad += call(bent.data(), L, 0, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    bent = ly;
    bent[(size_t)L - 1].stride_c = (long long)bent[(size_t)L - 1].H * bent[(size_t)L - 1].W - 1;
    bad += call(bent.data(), L, 0, H, ld, flags, top_k, ratio, 1) != FMPNP_EINVAL;
    if (bad) return fail(c, "argument errors", bad, -1);
    printf("ok   %-8s %s flags=%d  C=%d  N=%d  %d x %d x %d\n", c.name, ints ? "ints " : "reals", flags, C, N, B, H, W);
    return 0;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"equal", 1, 5, 3, 7, {{4, 5, 3}, {3, 5, 3}}, 0, true},
        {"dyadic", 2, 5, 3, 37, {{4, 5, 3}, {3, 5, 3}, {5, 3, 2}}, 2, true},
        {"ragged3", 1, 9, 7, 5, {{5, 9, 7}, {3, 5, 4}, {4, 3, 2}}, 0, false},
        {"blocks", 1, 4, 5, 3, {{70, 4, 5}, {3, 2, 3}, {64, 2, 2}}, 1, false},  // 137 = 2 * 64 + 9: a ragged last block
        {"line", 1, 1, 6, 4, {{4, 1, 6}, {3, 3, 3}}, 0, false},
        {"dot", 1, 3, 4, 4, {{3, 3, 4}, {5, 1, 1}}, 3, false},
        {"down", 1, 4, 3, 4, {{3, 4, 3}, {4, 9, 7}}, 0, false},
        {"batch3", 3, 9, 8, 6, {{5, 9, 8}, {3, 5, 4}}, 0, false},
        {"sized", 1, 7, 4, 4, {{4, 3, 5}, {2, 6, 2}}, 0, false},
        {"tiles2", 1, 24, 20, 129, {{33, 24, 20}, {40, 12, 10}}, 0, false},  // ragged channel counts, many rows
        {"long", 1, 40, 30, 2, {{3, 40, 30}, {2, 20, 15}}, 5, false},        // 1200 columns: two blocks of the chains
    };
    int failures = 0;
    for (const Case &c : cases)
        for (int ints = 0; ints <= 1; ++ints)
            for (int flags = 0; flags <= FMPNP_HC_NORMALIZE; ++flags) failures += run(c, ints != 0, flags);
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("layered match twin: all cases passed\n");
    return 0;
}
