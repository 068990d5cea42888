// Stand-alone host program over fmpnp_exhaustive_match_cpu / fmpnp_exhaustive_match_ex_cpu (fmpnp_match_cpu.cpp
// linked in), for sanitizer runs of the match stage's host code outside Python: `make match-sanitize` builds it
// with ASan + UBSan and runs it.  Exactly-sized heap operands with padded leading dimensions (a read one element
// past a row is an ASan report), both precisions, several thread counts; the f16 reference against a plain
// restatement (operands rounded to binary16 by the compiler's own _Float16 conversion, fp64 accumulation), the
// integers' exactness under both precisions, binary16 rounding at its edges, and the argument errors.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
float uni() { return (float)((double)rnd() / 2147483648.0 * 2.0 - 1.0); }

int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                           \
        }                                                      \
    } while (0)

float fl16(float x) { return (float)(_Float16)x; }  // (the compiler's conversion: nearest-even, subnormals kept)

struct Out {
    std::vector<int> argmax;
    std::vector<float> top, kth, scores;
    std::vector<unsigned char> mask;
    Out(int N, int WH) : argmax(N), top(N), kth(N), scores((size_t)N * WH), mask(N) {}
};

int run(const std::vector<float> &s, int N, int lds, const std::vector<float> &d, int C, int WH, int ldd, int top_k, Out &o,
        int threads, int precision) {
    return fmpnp_exhaustive_match_ex_cpu(s.data(), N, lds, d.data(), C, WH, ldd, top_k, 0.9, o.argmax.data(), o.top.data(),
                                         o.kth.data(), o.mask.data(), o.scores.data(), threads, precision);
}

void shape(int N, int C, int WH, bool ints) {
    const int lds = C + 3, ldd = WH + 5;
    // exactly sized: the last row ends at its last element, not at its leading dimension
    std::vector<float> s((size_t)(N - 1) * lds + C), d((size_t)(C - 1) * ldd + WH);
    for (auto &v : s) v = ints ? (float)((int)(rnd() % 5) - 2) : uni();
    for (auto &v : d) v = ints ? (float)((int)(rnd() % 5) - 2) : uni();
    const int top_k = WH > 7 ? 7 : 1;
    Out exact(N, WH), half(N, WH), again(N, WH);
    CHECK(run(s, N, lds, d, C, WH, ldd, top_k, exact, 1, FMPNP_MATCH_F32) == 0);
    CHECK(run(s, N, lds, d, C, WH, ldd, top_k, half, 3, FMPNP_MATCH_F16) == 0);
    CHECK(run(s, N, lds, d, C, WH, ldd, top_k, again, 0, FMPNP_MATCH_F16) == 0);
    CHECK(memcmp(half.scores.data(), again.scores.data(), half.scores.size() * 4) == 0);  // (any thread count)
    CHECK(half.argmax == again.argmax && half.mask == again.mask);
    {   // the twin entry point is the F32 precision
        Out twin(N, WH);
        CHECK(fmpnp_exhaustive_match_cpu(s.data(), N, lds, d.data(), C, WH, ldd, top_k, 0.9, twin.argmax.data(), twin.top.data(),
                                         twin.kth.data(), twin.mask.data(), twin.scores.data(), 2) == 0);
        CHECK(memcmp(twin.scores.data(), exact.scores.data(), twin.scores.size() * 4) == 0 && twin.argmax == exact.argmax);
    }
    for (int i = 0; i < N; ++i) {
        int best = 0;
        for (int j = 0; j < WH; ++j) {
            double acc = 0.0;
            for (int k = 0; k < C; ++k) acc += (double)fl16(s[(size_t)i * lds + k]) * (double)fl16(d[(size_t)k * ldd + j]);
            const float want = (float)acc, got = half.scores[(size_t)i * WH + j];
            CHECK(got == want);
            if (ints) CHECK(got == exact.scores[(size_t)i * WH + j]);
            if (got > half.scores[(size_t)i * WH + best]) best = j;
        }
        CHECK(half.argmax[i] == best && half.top[i] == half.scores[(size_t)i * WH + best]);
        CHECK(half.mask[i] == ((float)(0.9 * 0.9) * half.top[i] >= half.kth[i] ? 1 : 0));
    }
}

void rounding_edges() {
    const float vals[] = {1.0f + 0x1p-11f, 1.0f + 0x1.8p-10f, 0x1p-24f, 0x1p-25f, 0x1.8p-24f, 0x1p-14f - 0x1p-25f, 65504.0f,
                          65519.99f, 65520.0f, 1e5f, -1e5f, INFINITY, -INFINITY, 3e-9f, -0x1p-24f, 0x1.ffcp-15f, 0.33333334f};
    for (float v : vals) {
        std::vector<float> a(1, v), b(1, 1.0f);
        Out o(1, 1);
        CHECK(run(a, 1, 1, b, 1, 1, 1, 1, o, 1, FMPNP_MATCH_F16) == 0);
        CHECK(o.scores[0] == fl16(v));
        CHECK(run(b, 1, 1, a, 1, 1, 1, 1, o, 1, FMPNP_MATCH_F16) == 0);
        CHECK(o.scores[0] == fl16(v));
    }
    std::vector<float> a(1, NAN), b(1, 1.0f);
    Out o(1, 1);
    CHECK(run(a, 1, 1, b, 1, 1, 1, 1, o, 1, FMPNP_MATCH_F16) == 0);
    CHECK(o.scores[0] != o.scores[0] && o.top[0] != o.top[0] && o.argmax[0] == 0 && o.mask[0] == 0);
}

void errors() {
    std::vector<float> a(6, 1.0f), b(6, 1.0f);
    Out o(2, 2);
    CHECK(run(a, 2, 3, b, 3, 2, 2, 1, o, 1, 2) == FMPNP_EINVAL);   // an unknown precision
    CHECK(run(a, 2, 3, b, 3, 2, 2, 1, o, 1, -1) == FMPNP_EINVAL);
    CHECK(run(a, 2, 2, b, 3, 2, 2, 1, o, 1, FMPNP_MATCH_F16) == FMPNP_EINVAL);   // ld_sparse < C
    CHECK(run(a, 2, 3, b, 3, 2, 1, 1, o, 1, FMPNP_MATCH_F16) == FMPNP_EINVAL);   // ld_dense < WH
    CHECK(run(a, 2, 3, b, 3, 2, 2, 3, o, 1, FMPNP_MATCH_F16) == FMPNP_EINVAL);   // top_k > WH
    CHECK(run(a, 2, 3, b, 3, 2, 2, 1, o, -1, FMPNP_MATCH_F16) == FMPNP_EINVAL);  // n_threads < 0
    CHECK(run(a, 0, 3, b, 3, 2, 2, 1, o, 1, FMPNP_MATCH_F16) == 0);              // no rows: nothing is read
    CHECK(fmpnp_exhaustive_match_ex_cpu(nullptr, 2, 3, b.data(), 3, 2, 2, 1, 0.9, o.argmax.data(), o.top.data(), o.kth.data(),
                                        o.mask.data(), nullptr, 1, FMPNP_MATCH_F16) == FMPNP_EINVAL);
    CHECK(fmpnp_exhaustive_match_ex_cpu(a.data(), 2, 3, b.data(), 3, 2, 2, 1, 0.9, o.argmax.data(), o.top.data(), o.kth.data(),
                                        o.mask.data(), nullptr, 1, FMPNP_MATCH_F16) == 0);  // scores may be NULL
}

}  // namespace

int main() {
    shape(1, 1, 1, false);
    shape(37, 40, 480, false);
    shape(37, 40, 480, true);
    shape(5, 33, 1320, false);   // more than one column block of the accumulator
    shape(3, 1664, 130, true);
    rounding_edges();
    errors();
    printf(fails ? "test_match_cpu: %d check(s) FAILED\n" : "test_match_cpu: all checks passed\n", fails);
    return fails ? 1 : 0;
}
