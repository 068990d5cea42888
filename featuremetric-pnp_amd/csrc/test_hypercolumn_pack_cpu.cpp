// Stand-alone host program over fmpnp_hypercolumn_pack_cpu (fmpnp_hypercolumn_pack_cpu.cpp and the dense twin
// fmpnp_hypercolumn_cpu.cpp linked in), for sanitizer runs of the twin outside Python:
// `make hypercolumn-pack-sanitize` builds it with ASan + UBSan and runs it.  Seeded layers and exactly-sized heap
// buffers (a read or write one element outside a layer, the marks or the output is an ASan report).  The
// yardstick is the composed path on the host: the dense twin's map, then a Sobel written out here in the Sobel
// pack's association, rounded once.  Per case: both layouts, the four Sobel flag pairs, both storages, with and
// without the normalisation; ragged channel chunks and cstride > C; channel ranges; mark planes (random, empty,
// one texel); H = 1 and W = 1 outputs; 1 and 3 threads; untouched bytes (a sentinel everywhere else); the
// argument errors.
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

template <typename T>
bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0 || (a != a && b != b); }

const double SENTINEL = -7.0;

// the dense map's value with the Sobel's padding
double at(const std::vector<float> &m, int H, int W, int c, int y, int x, bool replicate) {
    if (y < 0 || y >= H || x < 0 || x >= W) {
        if (!replicate) return 0.0;
        y = y < 0 ? 0 : (y >= H ? H - 1 : y);
        x = x < 0 ? 0 : (x >= W ? W - 1 : x);
    }
    return (double)m[((size_t)c * H + y) * W + x];
}

template <typename T>
int check(const Case &c, const std::vector<fmpnp_hc_layer> &ly, int C, int item, int flags, bool grad, int sn, int rp,
          int c0, int c1, const std::vector<unsigned char> *marks, int dtype) {
    const int L = (int)ly.size(), H = c.H, W = c.W, cs = (C + 3) / 4 * 4, planes = grad ? 3 : 1;
    // the yardstick: the dense twin's map of this item
    std::vector<float> all((size_t)c.B * C * H * W);
    if (fmpnp_hypercolumn_assemble_cpu(ly.data(), L, c.B, all.data(), H, W, (long long)C * H * W, (long long)H * W, W,
                                       flags, 1)) {
        printf("FAIL %s: the dense twin refused the case\n", c.name);
        return 1;
    }
    const std::vector<float> m(all.begin() + (size_t)item * C * H * W, all.begin() + (size_t)(item + 1) * C * H * W);
    int bad = 0;
    for (int nt = 1; nt <= 3 && !bad; nt += 2) {
        std::vector<T> out((size_t)H * W * planes * cs, (T)SENTINEL);
        const int rc = fmpnp_hypercolumn_pack_cpu(ly.data(), L, c.B, item, H, W, flags, c0, c1,
                                                  grad ? FMPNP_LAYOUT_FGRAD : FMPNP_LAYOUT_F, dtype, cs, sn, rp,
                                                  marks ? marks->data() : nullptr, out.data(), nt);
        if (rc) {
            printf("FAIL %s: rc %d\n", c.name, rc);
            return 1;
        }
        for (int y = 0; y < H && !bad; ++y)
            for (int x = 0; x < W && !bad; ++x)
                for (int ch = 0; ch < cs && !bad; ++ch) {
                    const T *o = out.data() + ((size_t)y * W + x) * planes * cs + ch;
                    const bool written = ch >= c0 && ch < c1 && (!marks || (*marks)[(size_t)y * W + x]);
                    T want[3] = {(T)SENTINEL, (T)SENTINEL, (T)SENTINEL};
                    if (written) {
                        const bool r = rp != 0;
                        double a[3], d[3], g[3];
                        for (int j = 0; j < 3; ++j) {
                            a[j] = at(m, H, W, ch, y - 1, x - 1 + j, r);
                            d[j] = at(m, H, W, ch, y, x - 1 + j, r);
                            g[j] = at(m, H, W, ch, y + 1, x - 1 + j, r);
                        }
                        const double sxm = (a[0] + 2.0 * d[0]) + g[0], sxp = (a[2] + 2.0 * d[2]) + g[2];
                        const double sym = g[0] - a[0], sy0 = g[1] - a[1], syp = g[2] - a[2];
                        double gx = sxp - sxm, gy = (sym + 2.0 * sy0) + syp;
                        if (sn) {
                            gx *= 0.125;
                            gy *= 0.125;
                        }
                        want[0] = (T)m[((size_t)ch * H + y) * W + x];
                        want[1] = (T)gx;
                        want[2] = (T)gy;
                    }
                    for (int p = 0; p < planes; ++p)
                        if (!same_bits(o[(size_t)p * cs], want[p])) {
                            printf("FAIL %s: item %d flags %d grad %d sn %d rp %d range [%d, %d) marks %d dtype %d threads "
                                   "%d at (%d, %d) plane %d channel %d: %.17g, want %.17g\n",
                                   c.name, item, flags, (int)grad, sn, rp, c0, c1, marks ? 1 : 0, dtype, nt, y, x, p, ch,
                                   (double)o[(size_t)p * cs], (double)want[p]);
                            bad = 1;
                            break;
                        }
                }
    }
    return bad;
}

int run(const Case &c) {
    const int L = (int)c.layers.size();
    std::vector<std::vector<float>> data((size_t)L);
    std::vector<fmpnp_hc_layer> ly((size_t)L);
    int C = 0;
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
    std::vector<unsigned char> random((size_t)c.H * c.W), none((size_t)c.H * c.W, 0), one((size_t)c.H * c.W, 0);
    for (unsigned char &b : random) b = uni01() < 0.3 ? (unsigned char)(1 + (int)(uni01() * 200.0)) : 0;
    one[one.size() - 1] = 1;
    int bad = 0;
    for (int item = 0; item < c.B; ++item)
        for (int flags = 0; flags <= 1; ++flags) {
            bad |= check<float>(c, ly, C, item, flags, false, 0, 0, 0, C, nullptr, FMPNP_F32);
            for (int sn = 0; sn <= 1; ++sn)
                for (int rp = 0; rp <= 1; ++rp) {
                    bad |= check<float>(c, ly, C, item, flags, true, sn, rp, 0, C, nullptr, FMPNP_F32);
                    bad |= check<double>(c, ly, C, item, flags, true, sn, rp, 0, C, nullptr, FMPNP_F64);
                }
        }
    // ranges and marks (the last item, normalised)
    const int item = c.B - 1;
    const int mid = C / 2;
    const int ranges[3][2] = {{mid, C}, {0, mid > 0 ? mid : 1}, {C - 1, C}};
    for (const auto &r : ranges)
        for (int grad = 0; grad <= 1; ++grad)
            bad |= check<float>(c, ly, C, item, 1, grad != 0, 0, 1, r[0], r[1], nullptr, FMPNP_F32);
    for (const std::vector<unsigned char> *mk : {&random, &none, &one})
        for (int grad = 0; grad <= 1; ++grad) {
            bad |= check<float>(c, ly, C, item, 1, grad != 0, 1, 0, 0, C, mk, FMPNP_F32);
            bad |= check<float>(c, ly, C, item, 1, grad != 0, 0, 0, ranges[0][0], ranges[0][1], mk, FMPNP_F32);
        }
    bad |= check<double>(c, ly, C, item, 1, true, 0, 1, ranges[1][0], ranges[1][1], &random, FMPNP_F64);
    printf("%s %s\n", bad ? "FAIL" : "ok  ", c.name);
    return bad;
}

int argument_errors() {
    float src[2 * 3 * 3] = {0};
    fmpnp_hc_layer ok;
    memset(&ok, 0, sizeof ok);
    ok.data = src;
    ok.C = 2;
    ok.H = ok.W = 3;
    ok.stride_b = 18;
    ok.stride_c = 9;
    ok.stride_y = 3;
    std::vector<float> out((size_t)3 * 3 * 3 * 4, (float)SENTINEL);
    float *o = out.data();
    auto call = [&](const fmpnp_hc_layer *l, int L, int B, int item, int H, int W, int flags, int c0, int c1, int layout,
                    int dtype, int cs, void *dst, int nt) {
        return fmpnp_hypercolumn_pack_cpu(l, L, B, item, H, W, flags, c0, c1, layout, dtype, cs, 0, 0, nullptr, dst, nt);
    };
    int bad = 0;
    bad |= call(nullptr, 1, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 0, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 9, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 0, 0, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 1, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, -1, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 0, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 0, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 2, 0, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, -1, 2, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 1, 1, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 3, 0, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 2, 0, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 0, 2, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 0, 0, 1, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 1, 1, 4, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 1, 0, 6, o, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, nullptr, 1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, o, -1) != FMPNP_EINVAL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, (char *)o + 2, 1) != FMPNP_EALIGN;
    bad |= call(&ok, 1, 1, 0, 1 << 25, 3, 0, 0, 2, 0, 0, 4, o, 1) != FMPNP_ETOOBIG;
    for (float v : out) bad |= v != (float)SENTINEL;
    bad |= call(&ok, 1, 1, 0, 3, 3, 0, 0, 2, 0, 0, 4, o, 1) != 0;
    printf("%s argument errors\n", bad ? "FAIL" : "ok  ");
    return bad;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"ragged3", 1, 9, 7, {{5, 9, 7}, {3, 5, 4}, {4, 3, 2}}, 0},
        {"blocks", 1, 4, 5, {{70, 4, 5}, {3, 2, 3}, {64, 2, 2}}, 0},  // 137 channels: ragged chunks, cstride 140
        {"c30", 1, 6, 5, {{20, 6, 5}, {10, 3, 3}}, 0},                // cstride 32 > C
        {"cols33", 1, 3, 33, {{5, 3, 33}, {3, 2, 17}}, 0},
        {"rows", 1, 19, 4, {{4, 19, 4}, {3, 10, 2}}, 0},
        {"line", 1, 1, 6, {{4, 1, 6}, {3, 3, 3}}, 0},                 // H = 1
        {"column", 1, 5, 1, {{2, 5, 1}, {3, 2, 2}}, 0},               // W = 1
        {"one", 1, 1, 1, {{3, 1, 1}, {2, 2, 2}}, 0},                  // 1 x 1: every neighbour is padding
        {"sized", 1, 7, 4, {{4, 3, 5}, {2, 6, 2}}, 0},                // layer 0 resized too
        {"views", 2, 9, 8, {{5, 9, 8}, {3, 5, 4}, {4, 3, 2}}, 3},     // B = 2, padded source rows
    };
    int bad = 0;
    for (const Case &c : cases) bad |= run(c);
    bad |= argument_errors();
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad;
}
