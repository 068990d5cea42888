// Stand-alone host program over fmpnp_conv3x3_cpu / fmpnp_relu_cpu / fmpnp_maxpool2x2_cpu (fmpnp_encoder_cpu.cpp
// linked in), for sanitizer runs of the encoder's host code outside Python: `make encoder-sanitize` builds it with
// ASan + UBSan and runs it.  Every tensor is a heap block of exactly its size (a halo read one element outside the
// input is an ASan report).  The convolution on the test suite's small shapes, with and without bias and ReLU,
// against a plain restatement of the contract (one fmaf chain per output over k ascending, 0 for a tap outside),
// bit for bit and for several thread counts; small integers against exact fp64 sums; the ReLU and the pool at odd
// and even sizes with -0, negatives and NaN; the argument errors.
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

float relu(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }
bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

void conv_shape(int B, int Cin, int Cout, int H, int W, bool ints) {
    std::vector<float> in((size_t)B * Cin * H * W), w((size_t)Cout * Cin * 9), bias(Cout);
    for (auto &v : in) v = ints ? (float)((int)(rnd() % 5) - 2) : uni();
    for (auto &v : w) v = ints ? (float)((int)(rnd() % 3) - 1) : uni();
    for (auto &v : bias) v = ints ? (float)((int)(rnd() % 7) - 3) : uni();
    const size_t n_out = (size_t)B * Cout * H * W;
    for (int flags = 0; flags < 4; ++flags) {
        const bool has_bias = flags & FMPNP_CONV_BIAS, do_relu = flags & FMPNP_CONV_RELU;
        std::vector<float> got(n_out), again(n_out), want(n_out);
        CHECK(fmpnp_conv3x3_cpu(in.data(), B, Cin, H, W, w.data(), has_bias ? bias.data() : nullptr, Cout, flags, got.data(),
                                1) == 0);
        for (int threads : {0, 3}) {
            CHECK(fmpnp_conv3x3_cpu(in.data(), B, Cin, H, W, w.data(), has_bias ? bias.data() : nullptr, Cout, flags,
                                    again.data(), threads) == 0);
            CHECK(same_bits(got, again));  // (any thread count)
        }
        for (int b = 0; b < B; ++b)
            for (int co = 0; co < Cout; ++co)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        float acc = 0.f;
                        double exact = 0.0;
                        for (int ci = 0; ci < Cin; ++ci)
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx) {
                                    const int yy = y + ky - 1, xx = x + kx - 1;
                                    const float a = (yy >= 0 && yy < H && xx >= 0 && xx < W)
                                                        ? in[(((size_t)b * Cin + ci) * H + yy) * W + xx]
                                                        : 0.f;
                                    const float wk = w[((size_t)co * Cin + ci) * 9 + ky * 3 + kx];
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
                        const size_t o = (((size_t)b * Cout + co) * H + y) * W + x;
                        want[o] = acc;
                        if (ints) CHECK((double)got[o] == exact);
                    }
        CHECK(same_bits(got, want));
    }
}

void relu_and_pool(int H, int W) {
    const int B = 2, C = 3;
    std::vector<float> in((size_t)B * C * H * W);
    for (auto &v : in) v = uni();
    in[0] = -0.f;
    in[in.size() - 1] = NAN;
    if (in.size() > 4) in[1] = 0.f, in[2] = -3.f, in[3] = -0.f;
    std::vector<float> r(in.size());
    CHECK(fmpnp_relu_cpu(in.data(), r.data(), (long long)in.size(), 2) == 0);
    for (size_t i = 0; i < in.size(); ++i) {
        const float want = relu(in[i]);
        CHECK(memcmp(&r[i], &want, 4) == 0 && !(signbit(r[i]) && r[i] == 0.f));
    }
    std::vector<float> inplace(in);
    CHECK(fmpnp_relu_cpu(inplace.data(), inplace.data(), (long long)in.size(), 0) == 0 && same_bits(inplace, r));
    if (H < 2 || W < 2) {
        float dummy;
        CHECK(fmpnp_maxpool2x2_cpu(in.data(), B, C, H, W, &dummy, 1) == FMPNP_EINVAL);  // an empty output
        return;
    }
    const int OH = H / 2, OW = W / 2;
    std::vector<float> p((size_t)B * C * OH * OW), again(p.size());
    CHECK(fmpnp_maxpool2x2_cpu(in.data(), B, C, H, W, p.data(), 1) == 0);
    CHECK(fmpnp_maxpool2x2_cpu(in.data(), B, C, H, W, again.data(), 5) == 0 && same_bits(p, again));
    for (int pl = 0; pl < B * C; ++pl)
        for (int oy = 0; oy < OH; ++oy)
            for (int ox = 0; ox < OW; ++ox) {
                const float *q = in.data() + ((size_t)pl * H + 2 * oy) * W + 2 * ox;
                float m = q[0];
                for (float v : {q[1], q[W], q[W + 1]}) m = (v > m || v != v) ? v : m;
                const float got = p[((size_t)pl * OH + oy) * OW + ox];
                CHECK(memcmp(&got, &m, 4) == 0);
            }
}

void errors() {
    std::vector<float> in(2 * 9), w(2 * 9), bias(1), out(9);
    auto conv = [&](const float *i, int B, int Cin, int H, int W, const float *wt, const float *b, int Cout, int flags,
                    float *o, int t) { return fmpnp_conv3x3_cpu(i, B, Cin, H, W, wt, b, Cout, flags, o, t); };
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
    CHECK(conv(in.data(), 1, 1, 65536, 32768, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_ETOOBIG);  // 2^31 texels
    CHECK(conv(in.data(), 4, 2, 32768, 8192, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_ETOOBIG);
    CHECK(conv(in.data(), 1, 1, 3, 3, w.data(), nullptr, 1 << 30, 0, out.data(), 1) == FMPNP_ETOOBIG);
    CHECK(fmpnp_relu_cpu(nullptr, nullptr, 0, 1) == 0);
    CHECK(fmpnp_relu_cpu(nullptr, out.data(), 3, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_relu_cpu(in.data(), out.data(), -1, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_relu_cpu(in.data(), out.data(), 1ll << 31, 1) == FMPNP_ETOOBIG);
    CHECK(fmpnp_maxpool2x2_cpu(in.data(), 1, 2, 3, 3, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_maxpool2x2_cpu(in.data(), 1, 0, 3, 3, out.data(), 1) == FMPNP_EINVAL);
    CHECK(fmpnp_maxpool2x2_cpu(in.data(), 1, 2, 3, 1, out.data(), 1) == FMPNP_EINVAL);
    CHECK(fmpnp_maxpool2x2_cpu(in.data(), 1, 1, 65536, 32768, out.data(), 1) == FMPNP_ETOOBIG);
}

}  // namespace

int main() {
    const int shapes[][5] = {{1, 3, 5, 5, 7}, {1, 1, 1, 1, 1}, {2, 33, 130, 3, 131}, {1, 8, 64, 2, 258}, {3, 4, 4, 9, 4}};
    for (const auto &s : shapes) {
        conv_shape(s[0], s[1], s[2], s[3], s[4], false);
        conv_shape(s[0], s[1], s[2], s[3], s[4], true);
    }
    relu_and_pool(5, 7);
    relu_and_pool(1, 1);
    relu_and_pool(2, 258);
    errors();
    printf(fails ? "test_encoder_cpu: %d check(s) FAILED\n" : "test_encoder_cpu: all checks passed\n", fails);
    return fails ? 1 : 0;
}
