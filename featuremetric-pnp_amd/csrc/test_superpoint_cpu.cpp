// Stand-alone host program over the SuperPoint baseline's CPU twins (fmpnp_superpoint_cpu.cpp linked in), for
// sanitizer runs outside Python: `make superpoint-sanitize` builds it with ASan + UBSan and runs it.  Every
// buffer is an exactly-sized heap array (a read or write one element outside is an ASan report); the
// detector runs at sizes that are no multiple of anything, with keypoints on the map's edges so that the
// bilinear taps leave the map on every side; the NMS is compared with a plain restatement of the greedy walk,
// the matching and the assembly with plain loops; then the argument errors.
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
    errors();
    if (fails) {
        printf("test_superpoint_cpu: %d check(s) failed\n", fails);
        return 1;
    }
    printf("test_superpoint_cpu: ok\n");
    return 0;
}
