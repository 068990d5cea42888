// Stand-alone host program over fmpnp_hypercolumn_assemble_cpu (fmpnp_hypercolumn_cpu.cpp linked in), for
// sanitizer runs of the twin outside Python: `make hypercolumn-sanitize` builds it with ASan + UBSan and runs
// it.  It runs the shapes of tests/hypercolumn_cases.py with seeded values in exactly-sized heap buffers (so a
// read or write one element outside a layer or the output view is an ASan report), with 1 and 3 threads
// (the results must be equal), and the argument errors.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
float uni() {  // [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

struct Shape {
    int C, H, W;
};

struct Case {
    const char *name;
    int B, H, W;  // output size
    std::vector<Shape> layers;
    int pad;  // extra elements per source row (strided sources) and in front of the output (an unaligned view)
};

int run(const Case &c, int flags, int poison) {
    const int L = (int)c.layers.size();
    std::vector<std::vector<float>> data((size_t)L);
    std::vector<fmpnp_hc_layer> ly((size_t)L);
    long long C = 0;
    for (int l = 0; l < L; ++l) {
        const Shape &s = c.layers[(size_t)l];
        const long long sy = s.W + c.pad, sc = sy * s.H, sb = sc * s.C;
        // the last row of the last plane ends at its last texel: nothing behind it to read
        data[(size_t)l].resize((size_t)(sb * c.B - c.pad));
        for (float &v : data[(size_t)l]) v = uni();
        if (poison == 1)  // texel (0, 0) of every channel: the output's texel (0, 0) is zero in every channel
            for (int b = 0; b < c.B; ++b)
                for (int ch = 0; ch < s.C; ++ch) data[(size_t)l][(size_t)(b * sb + ch * sc)] = 0.0f;
        if (poison == 2 && l == L - 1) {
            data[(size_t)l][0] = NAN;
            data[(size_t)l][data[(size_t)l].size() - 1] = INFINITY;
        }
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
    const long long oy = c.W + c.pad, oc = oy * c.H, ob = oc * C;
    const size_t total = (size_t)(c.pad + ob * c.B - c.pad);
    std::vector<float> out1(total, -7.0f), out3(total, -7.0f);
    int rc = fmpnp_hypercolumn_assemble_cpu(ly.data(), L, c.B, out1.data() + c.pad, c.H, c.W, ob, oc, oy, flags, 1);
    rc |= fmpnp_hypercolumn_assemble_cpu(ly.data(), L, c.B, out3.data() + c.pad, c.H, c.W, ob, oc, oy, flags, 3);
    if (rc) {
        printf("%s: rc %d\n", c.name, rc);
        return 1;
    }
    if (memcmp(out1.data(), out3.data(), total * sizeof(float)) != 0) {
        printf("%s: 1 and 3 threads differ\n", c.name);
        return 1;
    }
    // outside the view nothing is written; inside, a normalised texel has unit length
    size_t bad = 0, nans = 0;
    for (size_t i = 0; i < total; ++i) {
        const long long j = (long long)i - c.pad;
        const bool inside = j >= 0 && j % oy < c.W;
        if (!inside && out1[i] != -7.0f) ++bad;
        if (inside && out1[i] != out1[i]) ++nans;
    }
    double worst = 0.0;
    if ((flags & FMPNP_HC_NORMALIZE) && poison == 0)
        for (int b = 0; b < c.B; ++b)
            for (int y = 0; y < c.H; ++y)
                for (int x = 0; x < c.W; ++x) {
                    double s = 0.0;
                    for (long long ch = 0; ch < C; ++ch) {
                        const double v = out1[(size_t)(c.pad + b * ob + ch * oc + y * oy + x)];
                        s += v * v;
                    }
                    worst = fmax(worst, fabs(s - 1.0));
                }
    printf("%s flags %d poison %d: C %lld, %zu NaN, |len^2 - 1| <= %.3g, %zu stray writes\n", c.name, flags, poison, C,
           nans, worst, bad);
    if (poison == 0 && nans) return 1;
    if (poison == 1 && (flags & FMPNP_HC_NORMALIZE) && nans != (size_t)(C * c.B)) return 1;
    return bad != 0 || !(worst < 1e-5);
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"ragged3", 1, 9, 7, {{5, 9, 7}, {3, 5, 4}, {4, 3, 2}}, 0},
        {"single", 1, 6, 5, {{7, 6, 5}}, 0},
        {"blocks", 1, 4, 5, {{70, 4, 5}, {3, 2, 3}, {64, 2, 2}}, 0},
        {"line", 1, 1, 6, {{4, 1, 6}, {3, 3, 3}}, 0},
        {"dot", 1, 3, 4, {{3, 3, 4}, {5, 1, 1}}, 0},
        {"down", 1, 4, 3, {{3, 4, 3}, {4, 9, 7}}, 0},
        {"wide", 1, 2, 257, {{3, 2, 257}, {2, 1, 129}}, 0},
        {"vgg16x", 1, 16, 16, {{128, 16, 16}, {256, 8, 8}, {256, 4, 4}, {512, 4, 4}, {512, 2, 2}}, 0},
        {"views", 2, 9, 8, {{5, 9, 8}, {3, 5, 4}, {4, 3, 2}}, 3},
    };
    int bad = 0;
    for (const Case &c : cases) {
        bad |= run(c, FMPNP_HC_NORMALIZE, 0);
        bad |= run(c, 0, 0);
    }
    bad |= run(cases[0], FMPNP_HC_NORMALIZE, 1);  // zero_texel
    bad |= run(cases[0], FMPNP_HC_NORMALIZE, 2);  // nonfinite
    bad |= run(cases[8], FMPNP_HC_NORMALIZE, 2);

    // argument errors: refused, nothing written
    float src[4] = {1, 2, 3, 4}, out[4] = {-7, -7, -7, -7};
    fmpnp_hc_layer ok = {src, 1, 2, 2, 0, 4, 4, 2};
    fmpnp_hc_layer many[9];
    for (fmpnp_hc_layer &m : many) m = ok;
    auto call = [&](const fmpnp_hc_layer *l, int L, int B, float *o, int H, int W, long long sy) {
        return fmpnp_hypercolumn_assemble_cpu(l, L, B, o, H, W, 4, 4, sy, FMPNP_HC_NORMALIZE, 1);
    };
    bad |= call(&ok, 1, 1, out, 2, 2, 2) != 0;
    for (float &v : out) v = -7.0f;
    bad |= call(&ok, 0, 1, out, 2, 2, 2) != FMPNP_EINVAL;
    bad |= call(many, 9, 1, out, 2, 2, 2) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 0, out, 2, 2, 2) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, out, 0, 2, 2) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, out, 2, 0, 2) != FMPNP_EINVAL;
    bad |= call(nullptr, 1, 1, out, 2, 2, 2) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, nullptr, 2, 2, 2) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, out, 2, 2, 1) != FMPNP_EINVAL;
    fmpnp_hc_layer broken = ok;
    broken.data = nullptr;
    bad |= call(&broken, 1, 1, out, 2, 2, 2) != FMPNP_EINVAL;
    broken = ok;
    broken.stride_y = 1;
    bad |= call(&broken, 1, 1, out, 2, 2, 2) != FMPNP_EINVAL;
    broken = ok;
    broken.C = 0;
    bad |= call(&broken, 1, 1, out, 2, 2, 2) != FMPNP_EINVAL;
    bad |= fmpnp_hypercolumn_assemble_cpu(&ok, 1, 1, out, 2, 2, 4, 4, 2, 8, 1) != FMPNP_EINVAL;
    for (float v : out) bad |= v != -7.0f;

    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
