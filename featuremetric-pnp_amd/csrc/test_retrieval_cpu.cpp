// Stand-alone host program over fmpnp_netvlad_pool_cpu and fmpnp_rank_topn_cpu (fmpnp_retrieval_cpu.cpp linked
// in), for sanitizer runs of the twins outside Python (`make retrieval-sanitize` builds it with ASan + UBSan
// and runs it) and for the sweep of the shared exponential (csrc/fmpnp_retrieval_impl.h exp_neg) against libm.
//
//   test_retrieval_cpu            the shapes of tests/retrieval_cases.py with seeded values in exactly-sized heap
//                                 buffers (a read or write one element outside is an ASan report), with 1 and 3
//                                 threads (the results must be equal), the ranking's order cases, the argument
//                                 errors, and the strided sweep
//   test_retrieval_cpu exp [S]    the sweep alone over every S-th float of [-104, 0] (default 64; 1: every
//                                 float, the run that FMPNP_NETVLAD_EXP_MAX_ULP records); prints exp_max_ulp=...
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_retrieval_impl.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
float uni() {  // [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++fails;                                                  \
        }                                                             \
    } while (0)

// the error of exp_neg in ulp of the exact value over every `stride`-th float of [-104, 0]
double exp_sweep(uint32_t stride, float *worst_x) {
    const uint32_t lo = 0x80000000u, hi = fmpnp::rv::float_bits(-104.0f);
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<double> worst(nt, 0.0);
    std::vector<float> at(nt, 0.f);
    std::vector<std::thread> threads;
    const uint64_t count = ((uint64_t)(hi - lo) + stride) / stride;
    for (unsigned t = 0; t < nt; ++t)
        threads.emplace_back([&, t]() {
            for (uint64_t i = count * t / nt; i < count * (t + 1) / nt; ++i) {
                const float x = fmpnp::rv::bits_float(lo + (uint32_t)(i * stride));
                const double ref = exp((double)x), got = (double)fmpnp::rv::exp_neg(x);
                int e;
                frexp(ref, &e);
                const double ulp = ldexp(1.0, std::max(e - 24, -149));
                const double err = fabs(got - ref) / ulp;
                if (err > worst[t]) {
                    worst[t] = err;
                    at[t] = x;
                }
            }
        });
    for (auto &th : threads) th.join();
    double w = 0.0;
    for (unsigned t = 0; t < nt; ++t)
        if (worst[t] > w) {
            w = worst[t];
            *worst_x = at[t];
        }
    return w;
}

struct Case {
    const char *name;
    int B, K, C, P;
    int pad;      // extra elements per channel row and per weight / centroid / output row
    int special;  // 1: an all-zero position and an all-zero image; 2: logits beyond +-200
};

void run_pool(const Case &c, int normalize) {
    const long long sc = c.P + c.pad, sb = sc * c.C;
    const int ld_w = c.C + c.pad, ld_c = c.C + c.pad;
    const long long ld_out = (long long)c.K * c.C + c.pad;
    // the last row of every array ends at its last element: nothing behind it to read or write
    std::vector<float> x((size_t)(sb * c.B - c.pad)), w((size_t)(ld_w * c.K - c.pad)), cent((size_t)(ld_c * c.K - c.pad));
    for (float &v : x) v = uni() * uni() * 4.f;
    for (float &v : w) v = uni() * (c.special == 2 ? 300.f : 20.f);
    for (float &v : cent) v = uni();
    if (c.special == 1) {
        for (int ch = 0; ch < c.C; ++ch) x[(size_t)(ch * sc + 1)] = 0.f;                                // position 1 of image 0
        for (int ch = 0; ch < c.C; ++ch)
            for (int p = 0; p < c.P; ++p) x[(size_t)((c.B - 1) * sb + ch * sc + p)] = 0.f;  // the last image
    }
    std::vector<float> o1((size_t)(ld_out * c.B - c.pad), -7.f), o3(o1);
    const int r1 = fmpnp_netvlad_pool_cpu(x.data(), c.B, c.C, c.P, sb, sc, w.data(), c.K, ld_w, cent.data(), ld_c,
                                          normalize, o1.data(), ld_out, 1);
    const int r3 = fmpnp_netvlad_pool_cpu(x.data(), c.B, c.C, c.P, sb, sc, w.data(), c.K, ld_w, cent.data(), ld_c,
                                          normalize, o3.data(), ld_out, 3);
    CHECK(r1 == 0 && r3 == 0);
    CHECK(memcmp(o1.data(), o3.data(), o1.size() * sizeof(float)) == 0);
    bool finite = true, pad_kept = true;
    for (int b = 0; b < c.B; ++b) {
        double ss = 0.0;
        for (long long i = 0; i < (long long)c.K * c.C; ++i) {
            const float v = o1[(size_t)(b * ld_out + i)];
            finite = finite && isfinite(v);
            ss += (double)v * v;
        }
        if (finite) CHECK(fabs(ss - 1.0) < 1e-5);
        if (b + 1 < c.B)
            for (int i = 0; i < c.pad; ++i) pad_kept = pad_kept && o1[(size_t)(b * ld_out + (long long)c.K * c.C + i)] == -7.f;
    }
    CHECK(finite);
    CHECK(pad_kept);
    // an image alone gives the bits it has in the batch
    std::vector<float> alone((size_t)c.K * c.C);
    const int b = c.B - 1;
    std::vector<float> xb(x.begin() + (size_t)(b * sb), x.end());
    CHECK(fmpnp_netvlad_pool_cpu(xb.data(), 1, c.C, c.P, sb, sc, w.data(), c.K, ld_w, cent.data(), ld_c, normalize,
                                 alone.data(), (long long)c.K * c.C, 2) == 0);
    CHECK(memcmp(alone.data(), &o1[(size_t)(b * ld_out)], alone.size() * sizeof(float)) == 0);
    printf("pool %-10s normalize=%d ok\n", c.name, normalize);
}

void run_rank() {
    const int Q = 7, D = 19, R = 45, n = 10;
    std::vector<float> q((size_t)Q * D), rt((size_t)D * R);
    for (float &v : q) v = uni();
    for (float &v : rt) v = uni();
    for (int d = 0; d < D; ++d) rt[(size_t)d * R + 30] = rt[(size_t)d * R + 4];  // a tie: reference 4 first
    q[(size_t)2 * D + 3] = NAN;                                                  // a NaN row: index order
    std::vector<int> i1((size_t)Q * n), i3(i1), iall((size_t)Q * R);
    std::vector<float> t1((size_t)Q * n), t3(t1), tall((size_t)Q * R), sc((size_t)Q * R);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R, n, i1.data(), t1.data(), nullptr, 1) == 0);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R, n, i3.data(), t3.data(), sc.data(), 3) == 0);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R, R, iall.data(), tall.data(), nullptr, 2) == 0);
    CHECK(i1 == i3 && memcmp(t1.data(), t3.data(), t1.size() * sizeof(float)) == 0);
    for (int qq = 0; qq < Q; ++qq) {
        for (int i = 0; i < n; ++i) CHECK(i1[(size_t)qq * n + i] == iall[(size_t)qq * R + i]);
        for (int i = 0; i + 1 < R; ++i) {
            const int a = iall[(size_t)qq * R + i], b = iall[(size_t)qq * R + i + 1];
            const float sa = sc[(size_t)qq * R + a], sb = sc[(size_t)qq * R + b];
            if (qq == 2)
                CHECK(a == i && sa != sa);
            else
                CHECK(sa > sb || (sa == sb && a < b));
        }
        int pos4 = -1, pos30 = -1;
        for (int i = 0; i < R; ++i) {
            if (iall[(size_t)qq * R + i] == 4) pos4 = i;
            if (iall[(size_t)qq * R + i] == 30) pos30 = i;
        }
        CHECK(qq == 2 || pos30 == pos4 + 1);
    }
    // argument errors
    int *ip = i1.data();
    float *tp = t1.data();
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R, 0, ip, tp, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R, R + 1, ip, tp, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D - 1, rt.data(), D, R, R, n, ip, tp, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R - 1, n, ip, tp, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_rank_topn_cpu(nullptr, Q, D, rt.data(), D, R, R, n, ip, tp, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, R, R, n, ip, tp, nullptr, -1) == FMPNP_EINVAL);
    CHECK(fmpnp_rank_topn_cpu(q.data(), Q, D, rt.data(), D, 1 << 20, 1 << 20, FMPNP_RANK_TOPN_CAP + 1, ip, tp, nullptr,
                              1) == FMPNP_ETOOBIG);
    CHECK(fmpnp_rank_topn_cpu(q.data(), 0, D, rt.data(), D, R, R, n, ip, tp, nullptr, 1) == 0);
    printf("rank ok\n");
}

void pool_errors() {
    float v[64] = {0};
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, v, 0, 2, v, 2, 1, v, 4, 1) == FMPNP_EINVAL);   // K < 1
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 2, v, 2, 2, v, 2, 1, v, 4, 1) == FMPNP_EINVAL);   // channel stride < P
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, v, 2, 1, v, 2, 1, v, 4, 1) == FMPNP_EINVAL);   // ld_w < C
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, v, 2, 2, v, 1, 1, v, 4, 1) == FMPNP_EINVAL);   // ld_c < C
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, v, 2, 2, v, 2, 1, v, 3, 1) == FMPNP_EINVAL);   // ld_out < K C
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, v, 2, 2, v, 2, 2, v, 4, 1) == FMPNP_EINVAL);   // the flag
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, nullptr, 2, 2, v, 2, 1, v, 4, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 3, 6, 3, v, 2, 2, v, 2, 1, v, 4, -1) == FMPNP_EINVAL);
    CHECK(fmpnp_netvlad_pool_cpu(v, 1, 2, 1 << 24, 1ll << 25, 1ll << 24, v, 2, 2, v, 2, 1, v, 4, 1) == FMPNP_ETOOBIG);
    CHECK(fmpnp_netvlad_pool_cpu(v, 0, 2, 3, 6, 3, v, 2, 2, v, 2, 1, v, 4, 1) == 0);
    printf("pool errors ok\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "exp") == 0) {
        const uint32_t stride = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 10) : 64u;
        float at = 0.f;
        const double w = exp_sweep(std::max(1u, stride), &at);
        printf("exp_max_ulp=%.4f at x=%.9g stride=%u\n", w, at, stride);
        return 0;
    }
    const Case cases[] = {
        {"small", 1, 8, 32, 35, 0, 0},       {"ragged", 1, 5, 24, 15, 0, 0},  {"batch3", 3, 8, 32, 35, 0, 0},
        {"views", 3, 5, 24, 15, 3, 0},       {"segments", 2, 6, 20, 2 * FMPNP_NETVLAD_SEGMENT + 5, 1, 0},
        {"zeros", 2, 8, 32, 35, 0, 1},       {"alpha", 1, 8, 32, 35, 0, 2},   {"k70", 1, 70, 130, 40, 0, 0},
    };
    for (const Case &c : cases)
        for (int normalize = 1; normalize >= 0; --normalize) run_pool(c, normalize);
    run_rank();
    pool_errors();
    float at = 0.f;
    const double w = exp_sweep(64, &at);
    printf("exp_max_ulp=%.4f at x=%.9g stride=64\n", w, at);
    CHECK(w <= (double)FMPNP_NETVLAD_EXP_MAX_ULP);
    CHECK(fmpnp::rv::exp_neg(0.f) == 1.f && fmpnp::rv::exp_neg(-INFINITY) == 0.f && isnan(fmpnp::rv::exp_neg(NAN)));
    printf(fails ? "%d checks FAILED\n" : "all ok\n", fails);
    return fails ? 1 : 0;
}
