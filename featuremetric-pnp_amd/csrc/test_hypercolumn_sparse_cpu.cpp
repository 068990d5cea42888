// Stand-alone host program over fmpnp_hypercolumn_sparse_cpu (fmpnp_hypercolumn_sparse_cpu.cpp and the dense
// twin fmpnp_hypercolumn_cpu.cpp linked in), for sanitizer runs of the twin outside Python:
// `make hypercolumn-sparse-sanitize` builds it with ASan + UBSan and runs it.  Seeded layers and exactly-sized
// heap buffers (a read or write one element outside a layer, the points or the output is an ASan report).  Per
// case: every texel (FMPNP_HC_AT_TEXEL) against the dense twin's map bit for bit; the two fp64 modes with points
// in and out of the map, NaN and huge coordinates and out-of-range items (error rows are zero, the others equal
// the dense map at the rule's texel); ld_out > C with the padding untouched; a ragged last block; N = 0; 1 and 3
// threads; both output types; the argument errors.
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
    int B, H, W;
    std::vector<Shape> layers;
    int pad;  // extra elements per source row
};

bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a != a && b != b); }

int fail(const Case &c, const char *what, long long p, long long ch) {
    printf("FAIL %s: %s at row %lld channel %lld\n", c.name, what, p, ch);
    return 1;
}

int run(const Case &c, int flags) {
    const int L = (int)c.layers.size();
    std::vector<std::vector<float>> data((size_t)L);
    std::vector<fmpnp_hc_layer> ly((size_t)L);
    long long C = 0;
    for (int l = 0; l < L; ++l) {
        const Shape &s = c.layers[(size_t)l];
        const long long sy = s.W + c.pad, sc = sy * s.H, sb = sc * s.C;
        data[(size_t)l].resize((size_t)(sb * c.B - c.pad));
        for (float &v : data[(size_t)l]) v = (float)(uni01() * 2.0 - 1.0);
        memset(&ly[(size_t)l], 0, sizeof ly[(size_t)l]);
        ly[(size_t)l].data = data[(size_t)l].data();
        ly[(size_t)l].C = s.C;
        ly[(size_t)l].H = s.H;
        ly[(size_t)l].W = s.W;
        ly[(size_t)l].stride_b = sb;
        ly[(size_t)l].stride_c = sc;
        ly[(size_t)l].stride_y = sy;
        C += s.C;
    }
    const int H = c.H, W = c.W, B = c.B;
    const size_t plane = (size_t)H * W;
    std::vector<float> dense((size_t)B * C * plane);
    if (fmpnp_hypercolumn_assemble_cpu(ly.data(), L, B, dense.data(), H, W, (long long)(C * plane), (long long)plane, W,
                                       flags, 2))
        return fail(c, "dense twin", -1, -1);
    auto at_dense = [&](int b, long long ch, int row, int col) {
        return dense[((size_t)b * C + (size_t)ch) * plane + (size_t)row * W + col];
    };

    // every texel of every item, rows of ld = C + 3 prefilled
    const int N = B * H * W;
    const long long ld = C + 3;
    std::vector<int> tex((size_t)N * 2), item((size_t)N);
    for (int p = 0; p < N; ++p) {
        item[(size_t)p] = p / (H * W);
        tex[2 * (size_t)p] = p % (H * W) / W;
        tex[2 * (size_t)p + 1] = p % W;
    }
    for (int threads = 1; threads <= 3; threads += 2) {
        std::vector<float> out((size_t)N * ld - 3, -7.0f);  // (the last row ends at its last channel)
        int flag = 0;
        const int rc = fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, tex.data(), item.data(), N, FMPNP_HC_AT_TEXEL,
                                                    0.0, 0.0, out.data(), FMPNP_F32, ld, flags, &flag, threads);
        if (rc || flag) return fail(c, "texel mode rc / flag", rc, flag);
        for (int p = 0; p < N; ++p) {
            for (long long ch = 0; ch < C; ++ch)
                if (!same_bits(out[(size_t)p * ld + ch], at_dense(item[(size_t)p], ch, tex[2 * (size_t)p], tex[2 * (size_t)p + 1])))
                    return fail(c, "texel mode value", p, ch);
            for (long long ch = C; ch < ld && p < N - 1; ++ch)
                if (out[(size_t)p * ld + ch] != -7.0f) return fail(c, "padding written", p, ch);
        }
    }

    // the fp64 modes: seeded points around the map, the deliberate bad ones, fp64 output
    const double img0 = 4.0 * H, img1 = 4.0 * W;  // rel0 = rel1 = 1 / 4: x spans the columns, y the rows
    const double cell0 = 3.5, cell1 = 2.25;
    const int M = 48;
    std::vector<double> pts((size_t)M * 2);
    std::vector<int> it((size_t)M);
    for (int p = 0; p < M; ++p) {
        pts[2 * (size_t)p] = (uni01() * 1.5 - 0.25) * 4.0 * W;
        pts[2 * (size_t)p + 1] = (uni01() * 1.5 - 0.25) * 4.0 * H;
        it[(size_t)p] = (int)(uni01() * B);
    }
    pts[0] = NAN;
    pts[3] = NAN;
    pts[4] = 1e300;
    pts[7] = -1e300;
    pts[8] = -1.5 * 4.0;  // (int)(-1.5) = -1 wraps to the last column
    pts[9] = 0.0;
    pts[10] = 4.0 * W - 1e-9;  // just inside the last texel
    pts[11] = 4.0 * H - 1e-9;
    pts[12] = cell1 * 2;  // exactly on a cell edge: the lower cell
    pts[13] = cell0;
    it[7] = B;  // out of range items
    it[8] = -1;
    for (int mode = FMPNP_HC_AT_REFERENCE; mode <= FMPNP_HC_AT_CELL; ++mode) {
        std::vector<double> out((size_t)M * C);
        int flag = 0;
        const bool ref = mode == FMPNP_HC_AT_REFERENCE;
        const int rc = fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, pts.data(), it.data(), M, mode, ref ? img0 : cell0,
                                                    ref ? img1 : cell1, out.data(), FMPNP_F64, C, flags, &flag, 2);
        int n_bad = 0;
        for (int p = 0; p < M; ++p) {
            const double x = pts[2 * (size_t)p], y = pts[2 * (size_t)p + 1];
            int row = -1, col = -1;
            bool ok = it[(size_t)p] >= 0 && it[(size_t)p] < B;
            if (ref) {  // the rule restated (include/fmpnp.h)
                const double cf = (double)H / img0 * x, rf = (double)W / img1 * y;
                if (!(fabs(cf) < 1e9 && fabs(rf) < 1e9)) ok = false;
                else {
                    col = (int)cf;
                    row = (int)rf;
                    if (row < 0 && row >= -H) row += H;
                    if (col < 0 && col >= -W) col += W;
                    if (row < 0 || row >= H || col < 0 || col >= W) ok = false;
                }
            } else {
                const double cc = ceil(x / cell1 - 1.0), rr = ceil(y / cell0 - 1.0);
                col = cc > 0.0 ? (cc < W - 1 ? (int)cc : W - 1) : 0;
                row = rr > 0.0 ? (rr < H - 1 ? (int)rr : H - 1) : 0;
            }
            n_bad += !ok;
            for (long long ch = 0; ch < C; ++ch) {
                const double got = out[(size_t)p * C + ch];
                if (!ok ? got != 0.0
                        : (!same_bits((float)got, at_dense(it[(size_t)p], ch, row, col)) || (double)(float)got != got))
                    return fail(c, ref ? "reference mode value" : "cell mode value", p, ch);
            }
        }
        if (n_bad < 2) return fail(c, "the bad points are missing", n_bad, mode);
        if (rc != FMPNP_ERANGE || flag != 1) return fail(c, "error rows without FMPNP_ERANGE / flag", rc, flag);
    }

    // N = 0 touches nothing (null buffers)
    if (fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, nullptr, nullptr, 0, FMPNP_HC_AT_TEXEL, 0.0, 0.0, nullptr,
                                     FMPNP_F32, C, flags, nullptr, 1))
        return fail(c, "N = 0", -1, -1);
    // argument errors
    float one[1];
    int t0[2] = {0, 0};
    int bad = 0;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, t0, nullptr, 1, FMPNP_HC_AT_TEXEL, 0, 0, one, FMPNP_F32, C - 1,
                                        flags, nullptr, 1) != FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, t0, nullptr, 1, 3, 0, 0, one, FMPNP_F32, C, flags, nullptr, 1) !=
           FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, t0, nullptr, 1, FMPNP_HC_AT_TEXEL, 0, 0, one, 2, C, flags, nullptr,
                                        1) != FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, t0, nullptr, 1, FMPNP_HC_AT_TEXEL, 0, 0, one, FMPNP_F32, C,
                                        flags | FMPNP_HC_VECTOR_STORES, nullptr, 1) != FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, t0, nullptr, 1, FMPNP_HC_AT_CELL, 0.0, 1.0, one, FMPNP_F32, C,
                                        flags, nullptr, 1) != FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), 0, B, H, W, t0, nullptr, 1, FMPNP_HC_AT_TEXEL, 0, 0, one, FMPNP_F32, C, flags,
                                        nullptr, 1) != FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, H, W, nullptr, nullptr, 1, FMPNP_HC_AT_TEXEL, 0, 0, one, FMPNP_F32, C,
                                        flags, nullptr, 1) != FMPNP_EINVAL;
    bad += fmpnp_hypercolumn_sparse_cpu(ly.data(), L, B, (1 << 24) + 1, W, t0, nullptr, 1, FMPNP_HC_AT_TEXEL, 0, 0, one,
                                        FMPNP_F32, C, flags, nullptr, 1) != FMPNP_ETOOBIG;
    if (bad) return fail(c, "argument errors", bad, -1);
    printf("ok   %-8s flags=%d  C=%lld  %d x %d x %d\n", c.name, flags, C, B, H, W);
    return 0;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"ragged3", 1, 9, 7, {{5, 9, 7}, {3, 5, 4}, {4, 3, 2}}, 0},
        {"blocks", 1, 4, 5, {{70, 4, 5}, {3, 2, 3}, {64, 2, 2}}, 0},  // 137 = 2 * 64 + 9: a ragged last block
        {"line", 1, 1, 6, {{4, 1, 6}, {3, 3, 3}}, 0},
        {"dot", 1, 3, 4, {{3, 3, 4}, {5, 1, 1}}, 0},
        {"down", 1, 4, 3, {{3, 4, 3}, {4, 9, 7}}, 0},
        {"batch3", 3, 9, 8, {{5, 9, 8}, {3, 5, 4}}, 0},
        {"strided", 2, 9, 8, {{5, 9, 8}, {3, 5, 4}, {4, 3, 2}}, 3},
        {"sized", 1, 7, 4, {{4, 3, 5}, {2, 6, 2}}, 0},
        {"chunks", 1, 2, 2, {{4100, 2, 2}, {90, 1, 1}}, 0},  // more channels than one chunk of the kernel's LDS
    };
    int failures = 0;
    for (const Case &c : cases)
        for (int flags = 0; flags <= FMPNP_HC_NORMALIZE; ++flags) failures += run(c, flags);
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("hypercolumn sparse twin: all cases passed\n");
    return 0;
}
