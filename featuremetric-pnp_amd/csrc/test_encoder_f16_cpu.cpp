// Stand-alone host program over the CPU side of the encoder's fp16 precision (fmpnp_encoder_cpu.cpp linked in):
// fmpnp_conv3x3_f16_cpu (the reference), fmpnp_conv3x3_pack_weights_f16_cpu and fmpnp_conv3x3_f16_weights_size, for
// sanitizer runs outside Python: `make encoder-f16-sanitize` builds it with ASan + UBSan and runs it.  Every tensor
// is a heap block of exactly its size (a read one element outside is an ASan report).  The reference on the test
// suite's shapes, with and without bias and ReLU, against a plain triple loop in fp64 over the operands rounded by
// the compiler's own _Float16 (within the roundings the contract names; bit for bit on small integers, where it also
// equals the exact twin), for several thread counts; the conversion at its boundaries; the weight pack's layout, its
// zero tails and its bytes against _Float16; the argument errors.
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
bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

void conv_shape(int B, int Cin, int Cout, int H, int W, bool ints) {
    std::vector<float> in((size_t)B * Cin * H * W), w((size_t)Cout * Cin * 9), bias(Cout);
    for (auto &v : in) v = ints ? (float)((int)(rnd() % 5) - 2) : uni();
    for (auto &v : w) v = ints ? (float)((int)(rnd() % 3) - 1) : uni();
    for (auto &v : bias) v = ints ? (float)((int)(rnd() % 7) - 3) : uni();
    const size_t n_out = (size_t)B * Cout * H * W;
    const double u = ldexp(1.0, -24);
    for (int flags = 0; flags < 4; ++flags) {
        const bool has_bias = flags & FMPNP_CONV_BIAS, do_relu = flags & FMPNP_CONV_RELU;
        const float *bp = has_bias ? bias.data() : nullptr;
        std::vector<float> got(n_out), again(n_out), exact32(n_out);
        CHECK(fmpnp_conv3x3_f16_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, got.data(), 1) == 0);
        for (int threads : {0, 3}) {
            CHECK(fmpnp_conv3x3_f16_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, again.data(), threads) == 0);
            CHECK(same_bits(got, again));  // (any thread count)
        }
        if (ints) {  // operands exact in fp16, sums exact in fp32: the exact twin's bits
            CHECK(fmpnp_conv3x3_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, exact32.data(), 1) == 0);
            CHECK(same_bits(got, exact32));
        }
        for (int b = 0; b < B; ++b)
            for (int co = 0; co < Cout; ++co)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        double s = 0.0, mag = 0.0;  // the plain triple loop: ci, ky, kx
                        for (int ci = 0; ci < Cin; ++ci)
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx) {
                                    const int yy = y + ky - 1, xx = x + kx - 1;
                                    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                                    const double a = (double)fl16(in[(((size_t)b * Cin + ci) * H + yy) * W + xx]);
                                    const double wk = (double)fl16(w[((size_t)co * Cin + ci) * 9 + ky * 3 + kx]);
                                    s += a * wk;
                                    mag += fabs(a * wk);
                                }
                        const double sb = has_bias ? s + (double)bias[co] : s;
                        const double want = do_relu ? (sb > 0.0 ? sb : 0.0) : sb;
                        // one rounding of s, one of the bias add, the two fp64 orders and the second-order terms
                        const double bnd = u * fabs(s) + (has_bias ? u * fabs(sb) : 0.0) +
                                           (2.0 * 9 * Cin * ldexp(1.0, -53) + ldexp(1.0, -47)) * mag;
                        const float g = got[(((size_t)b * Cout + co) * H + y) * W + x];
                        if (ints) CHECK((double)g == want);
                        else CHECK(fabs((double)g - want) <= bnd);
                        if (do_relu) CHECK(!(g < 0.f) && !(signbit(g) && g == 0.f));
                    }
    }
}

// 1 -> 1 channel, a 1 x 1 image, only the centre weight set: fl16(value), as the input and as the weight
void conversions() {
    const float pos[][2] = {{1.f + ldexpf(1.f, -11), 1.f},
                            {1.f + ldexpf(1.f, -11) + ldexpf(1.f, -23), 1.f + ldexpf(1.f, -10)},
                            {1.f + 3.f * ldexpf(1.f, -11), 1.f + ldexpf(1.f, -9)},
                            {65504.f, 65504.f},
                            {65519.99609375f, 65504.f},
                            {ldexpf(1.f, -14), ldexpf(1.f, -14)},
                            {ldexpf(1.f, -14) - ldexpf(1.f, -25), ldexpf(1.f, -14)},  // (a subnormal tie: to even, up)
                            {ldexpf(3.f, -25), ldexpf(1.f, -23)}};                    // 1.5 * 2^-24: a tie, to even (2)
    for (const auto &p : pos)
        for (float sign : {1.f, -1.f}) {
            const float value = sign * p[0], want = sign * p[1];
            CHECK(fl16(value) == want);  // (the expectation itself, by the compiler's _Float16)
            std::vector<float> x(1, value), one(9, 0.f), v(9, 0.f), unit(1, 1.f), out(1);
            one[4] = 1.f, v[4] = value;
            CHECK(fmpnp_conv3x3_f16_cpu(x.data(), 1, 1, 1, 1, one.data(), nullptr, 1, 0, out.data(), 1) == 0 && out[0] == want);
            CHECK(fmpnp_conv3x3_f16_cpu(unit.data(), 1, 1, 1, 1, v.data(), nullptr, 1, 0, out.data(), 1) == 0 && out[0] == want);
        }
}

void pack_shape(int Cin, int Cout) {
    std::vector<float> w((size_t)Cout * Cin * 9);
    for (auto &v : w) v = uni() * 3.f;
    w[0] = 65504.f, w[w.size() - 1] = -ldexpf(1.f, -14);
    if (w.size() > 4) w[1] = 1.f + ldexpf(1.f, -11), w[2] = -0.f, w[3] = ldexpf(1.f, -20);  // (a subnormal is kept)
    const size_t bytes = fmpnp_conv3x3_f16_weights_size(Cin, Cout);
    const int CB = (Cin + 15) / 16, rows = (Cout + 31) / 32 * 32;
    CHECK(bytes == (size_t)rows * CB * 9 * 16 * 2);
    // (operator new's blocks are 16-byte aligned, as the image must be; exactly `bytes` long)
    std::vector<_Float16> image(bytes / 2, (_Float16)7.f);
    CHECK(((uintptr_t)image.data() & 15) == 0);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), Cin, Cout, image.data()) == 0);
    for (int co = 0; co < rows; ++co)
        for (int cb = 0; cb < CB; ++cb)
            for (int t = 0; t < 9; ++t)
                for (int c = 0; c < 16; ++c) {
                    const int ci = 16 * cb + c;
                    const _Float16 want = (co < Cout && ci < Cin) ? (_Float16)w[((size_t)co * Cin + ci) * 9 + t] : (_Float16)0.f;
                    const _Float16 got = image[(((size_t)co * CB + cb) * 9 + t) * 16 + c];
                    CHECK(memcmp(&got, &want, 2) == 0);
                }
}

void errors() {
    std::vector<float> in(2 * 9), w(2 * 9), bias(1), out(9);
    std::vector<_Float16> image(32 * 9 * 16);
    auto conv = [&](const float *i, int B, int Cin, int H, int W, const float *wt, const float *b, int Cout, int flags,
                    float *o, int t) { return fmpnp_conv3x3_f16_cpu(i, B, Cin, H, W, wt, b, Cout, flags, o, t); };
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), bias.data(), 1, 3, out.data(), 1) == 0);
    CHECK(conv(in.data(), 0, 2, 3, 3, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 0, 3, 3, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 0, 3, w.data(), bias.data(), 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), bias.data(), 0, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), bias.data(), 1, 4, out.data(), 1) == FMPNP_EINVAL);  // an unknown flag
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, FMPNP_CONV_BIAS, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(nullptr, 1, 2, 3, 3, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, nullptr, nullptr, 1, 0, out.data(), 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, 0, nullptr, 1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 2, 3, 3, w.data(), nullptr, 1, 0, out.data(), -1) == FMPNP_EINVAL);
    CHECK(conv(in.data(), 1, 1, 65536, 32768, w.data(), nullptr, 1, 0, out.data(), 1) == FMPNP_ETOOBIG);  // 2^31 texels
    CHECK(conv(in.data(), 1, 1, 3, 3, w.data(), nullptr, 1 << 30, 0, out.data(), 1) == FMPNP_ETOOBIG);
    CHECK(conv(in.data(), 1, 1, 1, 1, w.data(), nullptr, 1 << 24, 0, out.data(), 1) == FMPNP_ETOOBIG);  // the padded image
    CHECK(fmpnp_conv3x3_f16_weights_size(0, 1) == 0 && fmpnp_conv3x3_f16_weights_size(1, 0) == 0);
    CHECK(fmpnp_conv3x3_f16_weights_size(1 << 15, 1 << 15) == 0 && fmpnp_conv3x3_f16_weights_size(1, 1 << 24) == 0);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), 2, 1, image.data()) == 0);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(nullptr, 2, 1, image.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), 2, 1, nullptr) == FMPNP_EINVAL);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), 2, 1, image.data() + 1) == FMPNP_EINVAL);  // not 16-byte aligned
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), 0, 1, image.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), 2, -1, image.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_conv3x3_pack_weights_f16_cpu(w.data(), 1, 1 << 24, image.data()) == FMPNP_ETOOBIG);
}

}  // namespace

int main() {
    // the shapes of tests/encoder_f16_cases.py
    const int shapes[][5] = {{1, 3, 5, 5, 7},  {1, 1, 1, 1, 1},  {2, 33, 130, 3, 131}, {1, 8, 64, 2, 258}, {3, 4, 4, 9, 4},
                             {1, 2, 65, 3, 5}, {1, 15, 3, 2, 5}, {1, 16, 3, 2, 5},     {1, 17, 3, 2, 5}};
    for (const auto &s : shapes) {
        conv_shape(s[0], s[1], s[2], s[3], s[4], false);
        conv_shape(s[0], s[1], s[2], s[3], s[4], true);
        pack_shape(s[1], s[2]);
    }
    conversions();
    errors();
    printf(fails ? "test_encoder_f16_cpu: %d check(s) FAILED\n" : "test_encoder_f16_cpu: all checks passed\n", fails);
    return fails ? 1 : 0;
}
