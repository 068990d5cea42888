// Stand-alone host program over the SuperPoint baseline's CPU twins (fmpnp_superpoint_cpu.cpp linked in), for
// sanitizer runs outside Python: `make superpoint-sanitize` builds it with ASan + UBSan and runs it.  Every
// buffer is an exactly-sized heap array (a read or write one element outside is an ASan report); the
// detector runs at sizes that are no multiple of anything, with keypoints on the map's edges so that the
// bilinear taps leave the map on every side; the NMS is compared with a plain restatement of the greedy walk,
// the matching and the assembly with plain loops; a plateau that fills a pts buffer of exactly the keep capacity,
// keypoints far off the map, huge, NaN and Inf, and an unordered match list with entries out of range; then the
// argument errors.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fmpnp.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
double uni() { return (double)rnd() / 2147483648.0; }
double gauss() { return sqrt(-2.0 * log(uni() + 1e-12)) * cos(6.283185307179586 * uni()); }

int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                              \
        }                                                         \
    } while (0)

void detector(int Hc, int Wc, int D, int d, double conf, int border) {
    const int H = 8 * Hc, W = 8 * Wc;
    std::vector<float> semi((size_t)65 * Hc * Wc), coarse((size_t)D * Hc * Wc), heat((size_t)H * W);
    for (float &v : semi) v = (float)(1.5 * gauss());
    for (float &v : coarse) v = (float)gauss();
    CHECK(fmpnp_sp_heatmap_cpu(semi.data(), Hc, Wc, heat.data()) == 0);
    for (int yc = 0; yc < Hc; ++yc)
        for (int xc = 0; xc < Wc; ++xc) {  // the cell's 64 heat values and the dustbin share sum to 1 - 1e-5 / s
            double s = 0, e64 = exp((double)semi[(size_t)64 * Hc * Wc + (size_t)yc * Wc + xc]), tot = e64;
            for (int c = 0; c < 64; ++c) {
                s += heat[(size_t)(8 * yc + c / 8) * W + 8 * xc + c % 8];
                tot += exp((double)semi[(size_t)c * Hc * Wc + (size_t)yc * Wc + xc]);
            }
            CHECK(fabs(s - (tot - e64) / (tot + 1e-5)) < 1e-5);
        }
    const long long cap = fmpnp_sp_nms_capacity(H, W, d);
    CHECK(cap == (long long)((H + d) / (d + 1)) * ((W + d) / (d + 1)));
    std::vector<double> pts((size_t)3 * cap);
    int n = -1;
    CHECK(fmpnp_sp_nms_cpu(heat.data(), H, W, conf, d, border, pts.data(), cap, &n) == 0);
    // the greedy walk restated: repeatedly the greatest remaining candidate
    std::vector<int> state((size_t)H * W);
    for (size_t i = 0; i < state.size(); ++i) state[i] = heat[i] >= (float)conf ? 1 : 0;
    int m = 0;
    for (;;) {
        long best = -1;
        for (long i = 0; i < (long)state.size(); ++i)
            if (state[i] == 1 && (best < 0 || heat[i] > heat[best])) best = i;
        if (best < 0) break;
        const int x = (int)(best % W), y = (int)(best / W);
        for (int v = std::max(0, y - d); v <= std::min(H - 1, y + d); ++v)
            for (int u = std::max(0, x - d); u <= std::min(W - 1, x + d); ++u)
                if (state[(size_t)v * W + u] == 1) state[(size_t)v * W + u] = 0;
        if (x < border || x >= W - border || y < border || y >= H - border) continue;
        CHECK(m < n && pts[m] == x && pts[cap + m] == y && pts[2 * cap + m] == (double)heat[best]);
        ++m;
    }
    CHECK(m == n);
    if (n <= 0) return;
    for (int align = 0; align < 2; ++align) {
        std::vector<float> desc((size_t)D * n);
        CHECK(fmpnp_sp_describe_cpu(coarse.data(), D, Hc, Wc, pts.data(), cap, n, H, W, align, desc.data(), n) == 0);
        for (int p = 0; p < n; ++p) {
            double s = 0;
            for (int c = 0; c < D; ++c) s += (double)desc[(size_t)c * n + p] * desc[(size_t)c * n + p];
            CHECK(fabs(s - 1.0) < 1e-5);
        }
    }
    // keypoints on and beyond the image's edges: every tap pattern of the zero padding
    const double edge[6][2] = {{0, 0}, {(double)W - 1, (double)H - 1}, {0, (double)H - 1}, {(double)W, (double)H},
                               {-9, 3}, {1e30, -1e30}};
    std::vector<double> ep(12);
    for (int p = 0; p < 6; ++p) {
        ep[p] = edge[p][0];
        ep[6 + p] = edge[p][1];
    }
    std::vector<float> desc((size_t)D * 6);
    CHECK(fmpnp_sp_describe_cpu(coarse.data(), D, Hc, Wc, ep.data(), 6, 6, H, W, 0, desc.data(), 6) == 0);
    CHECK(fmpnp_sp_describe_cpu(coarse.data(), D, Hc, Wc, ep.data(), 6, 6, H, W, 1, desc.data(), 6) == 0);
}

void matching(int N1, int N2, int D, double ratio, int M) {
    std::vector<float> d1((size_t)N1 * D), d2t((size_t)D * N2);
    for (float &v : d2t) v = (float)(gauss() / sqrt((double)D));
    for (int i = 0; i < N1; ++i) {
        const int j = (int)(rnd() % (uint32_t)N2);
        for (int k = 0; k < D; ++k)
            d1[(size_t)i * D + k] = i % 2 ? (float)(gauss() / sqrt((double)D)) : d2t[(size_t)k * N2 + j] + (float)(0.01 * gauss());
    }
    std::vector<int> idx((size_t)2 * N1);
    std::vector<float> dist((size_t)2 * N1);
    std::vector<unsigned char> ok((size_t)N1);
    std::vector<long long> matches((size_t)2 * N1);
    int n = -1;
    CHECK(fmpnp_sp_match_cpu(d1.data(), N1, D, d2t.data(), D, N2, N2, ratio, idx.data(), dist.data(), ok.data(),
                             matches.data(), &n) == 0);
    int seen = 0;
    for (int i = 0; i < N1; ++i) {
        CHECK(idx[2 * i] >= 0 && idx[2 * i] < N2 && idx[2 * i + 1] >= 0 && idx[2 * i + 1] < N2 && idx[2 * i] != idx[2 * i + 1]);
        CHECK(dist[2 * i] <= dist[2 * i + 1]);
        for (int j = 0; j < N2; ++j) {
            float s = 0.f;
            for (int k = 0; k < D; ++k) s = fmaf(d1[(size_t)i * D + k], d2t[(size_t)k * N2 + j], s);
            const float dd = 2.0f * (1.0f - s);
            if (j == idx[2 * i]) CHECK(dd == dist[2 * i]);
            if (j != idx[2 * i] && j != idx[2 * i + 1]) CHECK(dd >= dist[2 * i + 1]);
        }
        CHECK(ok[i] == (dist[2 * i] <= (float)(ratio * ratio) * dist[2 * i + 1] ? 1 : 0));
        if (ok[i]) {
            CHECK(seen < n && matches[2 * seen] == i && matches[2 * seen + 1] == idx[2 * i]);
            ++seen;
        }
    }
    CHECK(seen == n);
    // association and assembly on those matches
    std::vector<double> q((size_t)2 * N1), r((size_t)2 * N2), p2((size_t)2 * M), p3((size_t)3 * M);
    for (double &v : q) v = floor(1000 * uni());
    for (double &v : r) v = floor(1000 * uni());
    for (double &v : p2) v = 1000 * uni();
    for (double &v : p3) v = gauss();
    matches.resize((size_t)2 * n);
    std::vector<int> argmin((size_t)N2);
    std::vector<double> x2((size_t)2 * N2), r2((size_t)2 * N2), x3((size_t)3 * N2);
    int na = -1;
    CHECK(fmpnp_sp_assemble_cpu(q.data(), N1, N1, r.data(), N2, N2, p2.data(), p3.data(), M, matches.data(), n, argmin.data(),
                                x2.data(), r2.data(), x3.data(), &na) == 0);
    int row = 0;
    for (int i = 0; i < N2; ++i) {
        int best = 0;
        double bd = INFINITY;
        for (int m = 0; m < M; ++m) {
            const double dx = r[i] - p2[2 * m], dy = r[N2 + i] - p2[2 * m + 1], dd = dx * dx + dy * dy;
            if (dd < bd) {
                bd = dd;
                best = m;
            }
        }
        CHECK(argmin[i] == best);
        long long first = -1;
        for (int m = 0; m < n && first < 0; ++m)
            if (matches[2 * m + 1] == i) first = matches[2 * m];
        if (first < 0) continue;
        CHECK(row < na && x2[2 * row] == q[first] && x2[2 * row + 1] == q[N1 + first] && r2[2 * row] == r[i] &&
              r2[2 * row + 1] == r[N2 + i] && x3[3 * row + 2] == p3[3 * best + 2]);
        ++row;
    }
    CHECK(row == na);
}

// a plateau of equal heat keeps the lattice of multiples of d + 1 in pixel order: exactly the capacity, into a
// buffer of exactly that many columns
void plateau(int H, int W, int d) {
    std::vector<float> heat((size_t)H * W, 0.5f);
    const long long cap = fmpnp_sp_nms_capacity(H, W, d);
    std::vector<double> pts((size_t)3 * cap);
    int n = -1;
    CHECK(fmpnp_sp_nms_cpu(heat.data(), H, W, 0.25, d, 0, pts.data(), cap, &n) == 0);
    CHECK(n == cap);
    int m = 0;
    for (int y = 0; y < H; y += d + 1)
        for (int x = 0; x < W; x += d + 1, ++m)
            CHECK(m < n && pts[m] == x && pts[cap + m] == y && pts[2 * cap + m] == 0.5);
    CHECK(m == n);
    CHECK(fmpnp_sp_nms_cpu(heat.data(), H, W, 0.25, d, std::max(H, W), pts.data(), cap, &n) == 0 && n == 0);
}

// keypoints on, next to and far beyond every edge of the map, huge, NaN and Inf, with the map in an allocation of
// exactly its size: a tap read outside it is an ASan report.  A column without a tap is 0 / 0 in every channel
void off_map(int D, int Hc, int Wc) {
    const int H = 8 * Hc, W = 8 * Wc;
    std::vector<float> coarse((size_t)D * Hc * Wc);
    for (float &v : coarse) v = (float)gauss();
    const double w = W, h = H;
    const double xs[] = {0, 1, 3, 3.999, 4, w - 5, w - 4, w - 1, w, w + 3.5, w + 4.01, -3.9, -4.0, -4.5, -20, 1e30, NAN, 27.25, INFINITY};
    const double ys[] = {0, 1, 3, h + 3.5, 4, h - 5, h - 4, h - 1, h, 3.999, -3.9, h + 4.01, -4.0, -4.5, -20, 19.5, 1e30, NAN, INFINITY};
    const int N = (int)(sizeof(xs) / sizeof(xs[0]));
    std::vector<double> pts((size_t)2 * N);
    for (int p = 0; p < N; ++p) {
        pts[p] = xs[p];
        pts[N + p] = ys[p];
    }
    const int want_none[2] = {9, 5};
    for (int align = 0; align < 2; ++align) {
        std::vector<float> desc((size_t)D * N);
        CHECK(fmpnp_sp_describe_cpu(coarse.data(), D, Hc, Wc, pts.data(), N, N, H, W, align, desc.data(), N) == 0);
        int none = 0;
        for (int p = 0; p < N; ++p) {
            int nan = 0;
            double s = 0;
            for (int c = 0; c < D; ++c) {
                const float v = desc[(size_t)c * N + p];
                nan += v != v ? 1 : 0;
                s += (double)v * v;
            }
            CHECK(nan == 0 || nan == D);
            CHECK(nan == D || fabs(s - 1.0) < 1e-5);
            none += nan == D ? 1 : 0;
        }
        CHECK(none == want_none[align]);
    }
}

// equidistant and NaN landmarks, and an unordered match list with duplicates and entries outside the keypoints
void assembly_edges() {
    const int N1 = 40, N2 = 300, M = 260;
    std::vector<double> q((size_t)2 * N1), r((size_t)2 * N2), p2((size_t)2 * M), p3((size_t)3 * M);
    for (double &v : q) v = floor(500 * uni());
    for (double &v : r) v = floor(500 * uni());
    for (double &v : p2) v = floor(500 * uni()) + 0.5;
    for (double &v : p3) v = gauss();
    const int same[4] = {3, 67, 70, 200};
    for (int m : same) {
        p2[2 * m] = 250.5;
        p2[2 * m + 1] = 120.5;
    }
    p2[0] = p2[1] = p2[2] = p2[3] = NAN;  // landmarks 0 and 1 never win
    r[17] = 250.5, r[N2 + 17] = 120.5;
    r[18] = 251.5, r[N2 + 18] = 120.5;
    r[19] = NAN;
    std::vector<long long> matches;
    for (int k = 0; k < 120; ++k) {
        matches.push_back(rnd() % N1);
        matches.push_back(rnd() % N2);
    }
    const long long extra[][2] = {{31, 10},  {12, 10},  {7, 10},         {20, 255},        {5, 255},  {39, 256}, {0, 256},
                                  {8, 299},  {2, 299},  {-1, 12},        {N1, 13},         {4, N2},   {5, -5},   {1ll << 40, 14},
                                  {6, (1ll << 40) + 15}, {3, 11}, {3, 11}};
    for (const auto &e : extra) {
        matches.push_back(e[0]);
        matches.push_back(e[1]);
    }
    const int n = (int)(matches.size() / 2);
    std::vector<int> argmin((size_t)N2);
    std::vector<double> x2((size_t)2 * N2), r2((size_t)2 * N2), x3((size_t)3 * N2);
    int na = -1, row = 0;
    CHECK(fmpnp_sp_assemble_cpu(q.data(), N1, N1, r.data(), N2, N2, p2.data(), p3.data(), M, matches.data(), n, argmin.data(),
                                x2.data(), r2.data(), x3.data(), &na) == 0);
    CHECK(argmin[17] == 3 && argmin[18] == 3 && argmin[19] == 0);
    for (int i = 0; i < N2; ++i) {
        int best = 0;
        double bd = INFINITY;
        for (int m = M - 1; m >= 0; --m) {  // (descending: an equal distance at a lower index replaces)
            const double dx = r[i] - p2[2 * m], dy = r[N2 + i] - p2[2 * m + 1], dd = dx * dx + dy * dy;
            if (dd <= bd) {
                bd = dd;
                best = m;
            }
        }
        CHECK(argmin[i] == best);
        long long first = -1;
        for (int m = 0; m < n; ++m) {
            const long long a = matches[2 * m], b = matches[2 * m + 1];
            if (b == i && a >= 0 && a < N1 && (first < 0 || a < first)) first = a;
        }
        if (first < 0) continue;
        CHECK(row < na && x2[2 * row] == q[first] && x2[2 * row + 1] == q[N1 + first] && x3[3 * row] == p3[3 * best]);
        CHECK(r2[2 * row + 1] == r[N2 + i] && (r2[2 * row] == r[i] || i == 19));
        ++row;
    }
    CHECK(row == na);
    // one landmark, and none that is a number: landmark 0 for every keypoint
    CHECK(fmpnp_sp_assemble_cpu(q.data(), N1, N1, r.data(), N2, N2, p2.data() + 4, p3.data(), 1, matches.data(), 0, argmin.data(),
                                x2.data(), r2.data(), x3.data(), &na) == 0 && na == 0);
    for (int i = 0; i < N2; ++i) CHECK(argmin[i] == 0);
    std::vector<double> nans((size_t)2 * M, NAN);
    CHECK(fmpnp_sp_assemble_cpu(q.data(), N1, N1, r.data(), N2, N2, nans.data(), p3.data(), M, matches.data(), n, argmin.data(),
                                x2.data(), r2.data(), x3.data(), &na) == 0 && na == row);
    for (int i = 0; i < N2; ++i) CHECK(argmin[i] == 0);
}

void errors() {
    float f[8] = {0};
    double dd[8] = {0};
    long long mm[4] = {0, 0, 9, -1};
    int i4[4], n = -1;
    unsigned char b[2];
    CHECK(fmpnp_sp_heatmap_cpu(nullptr, 1, 1, f) == FMPNP_EINVAL && fmpnp_sp_heatmap_cpu(f, 0, 5, nullptr) == 0);
    CHECK(fmpnp_sp_nms_cpu(f, 1, 1, 0.5, FMPNP_SP_MAX_NMS_DIST + 1, 0, dd, 8, &n) == FMPNP_ETOOBIG);
    CHECK(fmpnp_sp_nms_cpu(f, 2, 2, 0.5, 0, 0, dd, 3, &n) == FMPNP_EINVAL);  // ld_pts below the capacity 4
    CHECK(fmpnp_sp_nms_cpu(f, 2, 2, -1.0, 0, 0, dd, 4, nullptr) == FMPNP_EINVAL);
    std::vector<double> p4(12);
    CHECK(fmpnp_sp_nms_cpu(f, 2, 2, -1.0, 0, 0, p4.data(), 4, &n) == 0 && n == 4);  // every pixel, equal heat: index order
    CHECK(p4[0] == 0 && p4[1] == 1 && p4[2] == 0 && p4[3] == 1 && p4[4] == 0 && p4[6] == 1);
    CHECK(fmpnp_sp_describe_cpu(f, 1, 1, 1, dd, 1, 1, 8, 8, 7, f, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_sp_describe_cpu(f, 1, 1, 1, dd, 0, 1, 8, 8, 0, f, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_sp_match_cpu(f, 1, 2, f, 2, 1, 1, 0.9, i4, f, b, mm, &n) == FMPNP_EINVAL);  // N2 < 2
    CHECK(fmpnp_sp_match_cpu(nullptr, 0, 2, nullptr, 2, 2, 2, 0.9, nullptr, nullptr, nullptr, nullptr, &n) == 0 && n == 0);
    CHECK(fmpnp_sp_match_cpu(f, 1, 2, f, 2, 2, 2, 0.9, i4, f, b, mm, nullptr) == FMPNP_EINVAL);
    // matches outside the keypoints are ignored; no landmark is an error
    double x2[4], r2[4], x3[6];
    CHECK(fmpnp_sp_assemble_cpu(dd, 2, 2, dd, 2, 2, dd, dd, 1, mm, 2, i4, x2, r2, x3, &n) == 0 && n == 1);
    CHECK(fmpnp_sp_assemble_cpu(dd, 2, 2, dd, 2, 2, dd, dd, 0, mm, 2, i4, x2, r2, x3, &n) == FMPNP_EINVAL);
    CHECK(fmpnp_sp_assemble_cpu(dd, 2, 2, dd, 0, 0, dd, dd, 0, mm, 2, i4, x2, r2, x3, &n) == 0 && n == 0);
    double nan2[2] = {NAN, NAN};
    CHECK(fmpnp_sp_assemble_cpu(dd, 0, 0, dd, 1, 1, nan2, dd, 1, nullptr, 0, i4, x2, r2, x3, &n) == 0 && n == 0 && i4[0] == 0);
}

}  // namespace

int main() {
    detector(3, 5, 20, 4, 0.01, 4);
    detector(7, 4, 70, 1, 0.005, 4);
    detector(2, 2, 64, 16, 0.001, 0);
    detector(4, 4, 8, 0, 0.03, 2);
    matching(2, 2, 5, 0.9, 1);
    matching(63, 65, 64, 0.9, 17);
    matching(257, 1025, 33, 0.7, 300);
    plateau(20, 37, 1);
    off_map(70, 5, 7);
    assembly_edges();
    errors();
    if (fails) {
        printf("test_superpoint_cpu: %d check(s) failed\n", fails);
        return 1;
    }
    printf("test_superpoint_cpu: ok\n");
    return 0;
}
