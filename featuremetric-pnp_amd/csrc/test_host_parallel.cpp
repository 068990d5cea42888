// Stand-alone host program over csrc/fmpnp_host.h, the CPU twins' shared plumbing: no GPU, no Python.
// `make host-sanitize` builds it once with ASan + UBSan and once with the thread sanitizer and runs both; the CPU
// tests run the plain build.
//
//   deal         every item of [0, n) exactly once for n in {0, 1, 3, 1000}, n_threads in {1, 2, 7, 0} and chunks of
//                1 and 64; a worker that throws on item 5, and a make_worker that throws on its second call, give
//                false with every thread joined (every worker state destroyed) and the program still running
//   fmaf_chains  the libm and the FMA version, and the one the picker resolves, are bit-equal to a scalar
//                std::fmaf loop on a 37 x 19 block (ld 23) with a subnormal, -0.f, an Inf and a NaN column
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <limits>
#include <new>
#include <vector>

#include "fmpnp_host.h"

namespace {

using namespace fmpnp::host;

int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++fails;                                                  \
        }                                                             \
    } while (0)

// a worker's state: counts itself in and out, so a zero after deal() shows that every thread was done with its
// worker (joined) before deal() returned
struct Live {
    std::atomic<int> *live;
    explicit Live(std::atomic<int> *l) : live(l) { ++*live; }
    Live(const Live &o) : live(o.live) { ++*live; }
    ~Live() { --*live; }
};

void test_coverage() {
    for (long long n : {0LL, 1LL, 3LL, 1000LL})
        for (int nt : {1, 2, 7, 0})
            for (long long chunk : {1LL, 64LL}) {
                std::vector<std::atomic<int>> seen((size_t)n);
                for (auto &s : seen) s = 0;
                std::atomic<int> live(0), workers(0);
                const bool ok = deal(n, nt, [&]() {
                    ++workers;
                    return [&seen, keep = Live(&live)](long long i) { ++seen[(size_t)i]; };
                }, chunk);
                CHECK(ok);
                CHECK(live == 0);
                CHECK(workers >= 1 && (nt == 0 || workers <= nt));
                CHECK(workers <= std::max<long long>(1, (n + chunk - 1) / chunk));  // (clamped to the chunks)
                bool once = true;
                for (auto &s : seen) once = once && s == 1;
                CHECK(once);
            }
}

void test_failures() {
    for (long long chunk : {1LL, 64LL}) {
        std::atomic<int> live(0);
        std::atomic<long long> visited(0);
        bool ok = deal(1000, 7, [&]() {
            return [&visited, keep = Live(&live)](long long i) {
                if (i == 5) throw std::bad_alloc();
                ++visited;
            };
        }, chunk);
        CHECK(!ok);
        CHECK(live == 0);
        CHECK(visited < 1000);
        // only the second make_worker fails: the other threads do all the work, and the call still reports it
        std::atomic<int> calls(0);
        visited = 0;
        ok = deal(1000, 3, [&]() {
            if (++calls == 2) throw std::bad_alloc();
            return [&visited, keep = Live(&live)](long long) { ++visited; };
        }, chunk);
        CHECK(!ok);
        CHECK(live == 0);
        CHECK(calls == 3 && visited == 1000);
    }
}

void test_chains() {
    constexpr int NI = 37, NJ = 19, LD = 23;
    std::vector<float> s(NI), m((size_t)NI * LD), want(NJ), got(NJ);
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto uni = [&rng]() {  // [-1, 1)
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((double)(rng >> 11) / 9007199254740992.0 * 2.0 - 1.0);
    };
    for (auto &v : s) v = uni();
    for (auto &v : m) v = uni();
    s[2] = 1e-41f;                                              // a subnormal factor
    s[20] = -0.f;
    m[(size_t)6 * LD + 11] = 1e-40f;                            // ... and a subnormal entry
    for (int i = 0; i < NI; ++i) m[(size_t)i * LD + 5] = -0.f;  // a column whose chain stays a signed zero
    m[(size_t)4 * LD + 3] = std::numeric_limits<float>::infinity();
    m[(size_t)20 * LD + 3] = std::numeric_limits<float>::infinity();  // (Inf x -0: the column ends as NaN)
    m[(size_t)10 * LD + 7] = std::numeric_limits<float>::quiet_NaN();
    for (int j = 0; j < NJ; ++j) {
        float acc = 0.f;
        for (int i = 0; i < NI; ++i) acc = std::fmaf(s[i], m[(size_t)i * LD + j], acc);
        want[j] = acc;
    }
    CHECK(std::isnan(want[3]) && std::isnan(want[7]) && want[5] == 0.f);
    auto same = [&](fmaf_chains_fn fn) {
        std::fill(got.begin(), got.end(), 123.f);  // (the chains start from +0 whatever acc held)
        fn(s.data(), m.data(), LD, NI, NJ, got.data());
        return memcmp(got.data(), want.data(), sizeof(float) * NJ) == 0;
    };
    CHECK(same(fmaf_chains_libm));
    CHECK(same(fmaf_chains));
#if defined(__x86_64__)
    if (have_fma()) CHECK(same(fmaf_chains_fma));
    else printf("fmaf_chains_fma skipped: this core has no FMA\n");
#else
    printf("fmaf_chains_fma skipped: not built for this architecture\n");
#endif
}

}  // namespace

int main() {
    test_coverage();
    test_failures();
    test_chains();
    if (fails) {
        printf("%d checks FAILED\n", fails);
        return 1;
    }
    printf("all ok\n");
    return 0;
}
