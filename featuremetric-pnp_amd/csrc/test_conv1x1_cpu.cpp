// Stand-alone host program over fmpnp_conv1x1_cpu (fmpnp_conv1x1_cpu.cpp linked in), for sanitizer runs of the 1x1
// convolution's host code outside Python: `make conv1x1-sanitize` builds it with ASan + UBSan and runs it.  The
// input, the weights and the bias are heap blocks of exactly their size (a read one element outside is an ASan
// report); the output lies between two guard bands of NaN that must stay NaN.  The twin on the test suite's ragged
// shapes, with and without bias and ReLU: against a plain restatement of the contract (one fmaf chain per output
// over ci ascending), bit for bit and for several thread counts; on small integers against a plain double-precision
// loop, exactly; the argument errors.
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

constexpr size_t GUARD = 64;

float relu(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }
bool guards_intact(const std::vector<float> &buf) {
    for (size_t i = 0; i < GUARD; ++i)
        if (buf[i] == buf[i] || buf[buf.size() - 1 - i] == buf[buf.size() - 1 - i]) return false;
    return true;
}

void conv_shape(int B, int Cin, int Cout, int H, int W, bool ints) {
    const size_t hw = (size_t)H * W, n_out = (size_t)B * Cout * hw;
    std::vector<float> in((size_t)B * Cin * hw), w((size_t)Cout * Cin), bias(Cout);
    for (auto &v : in) v = ints ? (float)((int)(rnd() % 5) - 2) : uni();
    for (auto &v : w) v = ints ? (float)((int)(rnd() % 3) - 1) : uni();
    for (auto &v : bias) v = ints ? (float)((int)(rnd() % 7) - 3) : uni();
    for (int flags = 0; flags < 4; ++flags) {
        const bool has_bias = flags & FMPNP_CONV_BIAS, do_relu = flags & FMPNP_CONV_RELU;
        const float *bp = has_bias ? bias.data() : nullptr;
        std::vector<float> got(n_out + 2 * GUARD, NAN), again(n_out + 2 * GUARD, NAN);
        CHECK(fmpnp_conv1x1_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, got.data() + GUARD, 1) == 0);
        CHECK(guards_intact(got));
        for (int threads : {0, 3}) {
            CHECK(fmpnp_conv1x1_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, again.data() + GUARD, threads) == 0);
            CHECK(guards_intact(again));
            CHECK(memcmp(got.data() + GUARD, again.data() + GUARD, n_out * 4) == 0);  // (any thread count)
        }
        for (int b = 0; b < B; ++b)
            for (int co = 0; co < Cout; ++co)
                for (size_t p = 0; p < hw; ++p) {
                    float acc = 0.f;
                    double exact = 0.0;
                    for (int ci = 0; ci < Cin; ++ci) {
                        const float a = in[((size_t)b * Cin + ci) * hw + p], wk = w[(size_t)co * Cin + ci];
                        acc = fmaf(a, wk, acc);
                        exact += (double)a * (double)wk;
                    }
                    if (has_bias) {
                        volatile float s = acc + bias[co];  // (its own rounding)
                        acc = s;
                        exact += (double)bias[co];
                    }
                    if (do_relu) {
                        acc = relu(acc);
                        exact = exact > 0.0 ? exact : 0.0;
                    }
                    const float g = got[GUARD + ((size_t)b * Cout + co) * hw + p];
                    CHECK(memcmp(&g, &acc, 4) == 0);
                    if (ints) CHECK((double)g == exact);
                }
    }
}

void errors() {
    std::vector<float> in(2 * 9), w(2), bias(1), out(9);
    auto conv = [&](const float *i, int B, int Cin, int H, int W, const float *wt, const float *b, int Cout, int flags,
                    float *o, int t) { return fmpnp_conv1x1_cpu(i, B, Cin, H, W, wt, b, Cout, flags, o, t); };
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), bias.data(), 1, 3, out.data(), 1) == 0);
    CHECK(conv(in.data(), 0, 2, 3, 3, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 0, 3, 3, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 0, 3, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, -1, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), bias.data(), 0, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), bias.data(), 1, 4, out.data(), 1) == FMPNP_EINVAL);   // an unknown flag
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, FMPNP_CONV_BIAS, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, 0, out.data(), 1) == 0);                  // no bias asked for
    CHECK(conv(nullptr, 1, 2, 3, 3, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, nullptr, nullptr, 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, 0, nullptr, 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, 0, out.data(), -1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 1, 65536, 32768, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_ETOOBIG);  // 2^31 pixels
    CHECK(conv(in.data(), 4, 2, 32768, 8192, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_ETOOBIG);   // the input
    CHECK(conv(in.data(), 1, 1, 3, 3, w.data(), nullptr, 1 << 30, 0, out.data(), 1) == FMPNP_ETOOBIG);    // the output
    CHECK(conv(in.data(), 1, 1 << 16, 1, 1, w.data(), nullptr, 1 << 15, 0, out.data(), 1) == FMPNP_ETOOBIG);  // the weights
}

}  // namespace

int main() {
    const int shapes[][5] = {{1, 1, 1, 1, 1},   {1, 3, 5, 5, 7},  {2, 33, 130, 3, 131}, {1, 8, 64, 2, 258},
                             {1, 2, 65, 3, 5},  {3, 70, 4, 9, 4}, {1, 256, 65, 2, 3},   {1, 256, 256, 2, 3},
                             {1, 5, 66, 4, 33}};
    for (const auto &s : shapes) {
        conv_shape(s[0], s[1], s[2], s[3], s[4], false);
        conv_shape(s[0], s[1], s[2], s[3], s[4], true);
    }
    errors();
    printf(fails ? "test_conv1x1_cpu: %d check(s) FAILED\n" : "test_conv1x1_cpu: all checks passed\n", fails);
    return fails ? 1 : 0;
}
