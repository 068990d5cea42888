// Stand-alone host program over the dense-feature twins (fmpnp_dense_cpu.cpp and fmpnp_encoder_cpu.cpp linked in), for
// sanitizer runs of their host code outside Python: `make dense-sanitize` builds it with ASan + UBSan and runs it.
// Every input is a heap block of exactly its size (a read one element outside is an ASan report); every output lies
// between two guard bands of NaN that must stay NaN.  fmpnp_conv3x3_dilated_cpu at dilation 1 and 2 on the test
// suite's small shapes against a plain restatement of the contract (one fmaf chain per output over k ascending, a tap
// off the map the operand 0), bit for bit, and at dilation 1 against fmpnp_conv3x3_cpu; fmpnp_avgpool2x2s1_cpu against
// its expression and, on integers, exactly; fmpnp_dense_pyramid_step_cpu against a plain restatement (the bilinear
// taps, one add, fp64 block sums, the clamped division), in place too; the argument errors.
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

void conv_shape(int B, int Cin, int Cout, int H, int W, int d, bool ints) {
    const size_t hw = (size_t)H * W, n_out = (size_t)B * Cout * hw;
    std::vector<float> in((size_t)B * Cin * hw), w((size_t)Cout * Cin * 9), bias(Cout);
    for (auto &v : in) v = ints ? (float)((int)(rnd() % 5) - 2) : uni();
    for (auto &v : w) v = ints ? (float)((int)(rnd() % 3) - 1) : uni();
    for (auto &v : bias) v = ints ? (float)((int)(rnd() % 7) - 3) : uni();
    for (int flags = 0; flags < 4; ++flags) {
        const bool has_bias = flags & FMPNP_CONV_BIAS, do_relu = flags & FMPNP_CONV_RELU;
        const float *bp = has_bias ? bias.data() : nullptr;
        std::vector<float> got(n_out + 2 * GUARD, NAN), again(n_out + 2 * GUARD, NAN);
        CHECK(fmpnp_conv3x3_dilated_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, got.data() + GUARD, d, 1) == 0);
        CHECK(guards_intact(got));
        CHECK(fmpnp_conv3x3_dilated_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, again.data() + GUARD, d, 3) == 0);
        CHECK(guards_intact(again));
        CHECK(memcmp(got.data() + GUARD, again.data() + GUARD, n_out * 4) == 0);  // (any thread count)
        if (d == 1) {  // the undilated twin's bits
            std::vector<float> plain(n_out + 2 * GUARD, NAN);
            CHECK(fmpnp_conv3x3_cpu(in.data(), B, Cin, H, W, w.data(), bp, Cout, flags, plain.data() + GUARD, 2) == 0);
            CHECK(guards_intact(plain));
            CHECK(memcmp(got.data() + GUARD, plain.data() + GUARD, n_out * 4) == 0);
        }
        for (int b = 0; b < B; ++b)
            for (int co = 0; co < Cout; ++co)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        float acc = 0.f;
                        double exact = 0.0;
                        for (int k = 0; k < 9 * Cin; ++k) {
                            const int ci = k / 9, ky = k % 9 / 3, kx = k % 3, yy = y + (ky - 1) * d, xx = x + (kx - 1) * d;
                            const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
                            const float a = inside ? in[((size_t)b * Cin + ci) * hw + (size_t)yy * W + xx] : 0.f;
                            const float wk = w[(size_t)co * Cin * 9 + k];
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
                        const float g = got[GUARD + ((size_t)b * Cout + co) * hw + (size_t)y * W + x];
                        CHECK(memcmp(&g, &acc, 4) == 0);
                        if (ints) CHECK((double)g == exact);
                    }
    }
}

void pool_shape(int B, int C, int H, int W, bool ints) {
    const size_t n_out = (size_t)B * C * (H - 1) * (W - 1);
    std::vector<float> in((size_t)B * C * H * W);
    for (auto &v : in) v = ints ? (float)((int)(rnd() % 17) - 8) : uni();
    std::vector<float> got(n_out + 2 * GUARD, NAN), again(n_out + 2 * GUARD, NAN);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), B, C, H, W, got.data() + GUARD, 1) == 0);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), B, C, H, W, again.data() + GUARD, 3) == 0);
    CHECK(guards_intact(got) && guards_intact(again));
    CHECK(memcmp(got.data() + GUARD, again.data() + GUARD, n_out * 4) == 0);
    size_t i = GUARD;
    for (int p = 0; p < B * C; ++p)
        for (int y = 0; y + 1 < H; ++y)
            for (int x = 0; x + 1 < W; ++x, ++i) {
                const float *r0 = in.data() + ((size_t)p * H + y) * W + x, *r1 = r0 + W;
                volatile float s = r0[0] + r0[1];
                s = s + r1[0];
                s = s + r1[1];
                const float want = s * 0.25f;
                CHECK(memcmp(&got[i], &want, 4) == 0);
                if (ints) CHECK((double)got[i] == ((double)r0[0] + r0[1] + r1[0] + r1[1]) / 4.0);
            }
}

struct Tap {
    int i0, i1;
    float w0, w1;
};
Tap tap_of(int n_in, int n_out, int d) {  // the assembly's align_corners=True taps, restated
    const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f;
    volatile float src = scale * (float)d;
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > n_in - 1) t.i0 = n_in - 1;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    volatile float w1 = src - (float)t.i0;
    volatile float w0 = 1.0f - w1;
    t.w1 = w1;
    t.w0 = w0;
    return t;
}
float mul(float a, float b) {
    volatile float r = a * b;
    return r;
}
float add(float a, float b) {
    volatile float r = a + b;
    return r;
}

void step_shape(int B, int C, int h, int w, int hp, int wp, bool with_prev, bool norm, bool zero_column) {
    const size_t n = (size_t)B * C * h * w;
    std::vector<float> cur(n), prev(with_prev ? (size_t)B * C * hp * wp : 1);
    for (auto &v : cur) v = uni();
    for (auto &v : prev) v = uni();
    if (zero_column) {  // texel (0, 0) of image 0: every channel 0 in cur, and prev all zero
        for (auto &v : prev) v = 0.f;
        for (int c = 0; c < C; ++c) cur[(size_t)c * h * w] = 0.f;
    }
    const float *pp = with_prev ? prev.data() : nullptr;
    const int flags = norm ? FMPNP_PYR_NORMALIZE : 0;
    std::vector<float> got(n + 2 * GUARD, NAN), again(n + 2 * GUARD, NAN);
    CHECK(fmpnp_dense_pyramid_step_cpu(cur.data(), pp, B, C, h, w, hp, wp, got.data() + GUARD, flags, 1) == 0);
    CHECK(guards_intact(got));
    // in place (out == cur), several threads
    memcpy(again.data() + GUARD, cur.data(), n * 4);
    CHECK(fmpnp_dense_pyramid_step_cpu(again.data() + GUARD, pp, B, C, h, w, hp, wp, again.data() + GUARD, flags, 3) == 0);
    CHECK(guards_intact(again));
    CHECK(memcmp(got.data() + GUARD, again.data() + GUARD, n * 4) == 0);
    std::vector<float> v(C);
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                for (int c = 0; c < C; ++c) {
                    float val = cur[(((size_t)b * C + c) * h + y) * w + x];
                    if (with_prev) {
                        const Tap ty = tap_of(hp, h, y), tx = tap_of(wp, w, x);
                        const float *pl = prev.data() + ((size_t)b * C + c) * hp * wp;
                        const float *r0 = pl + (size_t)ty.i0 * wp, *r1 = pl + (size_t)ty.i1 * wp;
                        const float top = add(mul(tx.w0, r0[tx.i0]), mul(tx.w1, r0[tx.i1]));
                        const float bot = add(mul(tx.w0, r1[tx.i0]), mul(tx.w1, r1[tx.i1]));
                        val = add(val, add(mul(ty.w0, top), mul(ty.w1, bot)));
                    }
                    v[c] = val;
                }
                float dv = 1.f;
                if (norm) {
                    double sum = 0.0;
                    for (int c0 = 0; c0 < C; c0 += 64) {
                        double acc = 0.0;
                        for (int c = c0; c < C && c < c0 + 64; ++c) acc = fma((double)v[c], (double)v[c], acc);
                        sum = sum + acc;
                    }
                    dv = (float)sqrt(sum);
                    if (dv < 1e-12f) dv = 1e-12f;
                }
                for (int c = 0; c < C; ++c) {
                    volatile float q = norm ? v[c] / dv : v[c];
                    const float want = q, g = got[GUARD + (((size_t)b * C + c) * h + y) * w + x];
                    CHECK(memcmp(&g, &want, 4) == 0);
                    if (zero_column && norm && b == 0 && y == 0 && x == 0) CHECK(g == 0.f && !signbit(g));
                }
            }
}

void errors() {
    std::vector<float> in(2 * 9), w(2 * 9), bias(1), out(2 * 9);
    auto conv = [&](int Cin, int H, int W, int flags, const float *b, int d, int t) {
        return fmpnp_conv3x3_dilated_cpu(in.data(), 1, Cin, H, W, w.data(), b, 1, flags, out.data(), d, t);
    };
    CHECK(conv(2, 3, 3, 3, bias.data(), 2, 1) == 0);
    CHECK(conv(2, 3, 3, 3, bias.data(), 1, 1) == 0);
    for (int d : {0, 3, -1, 4}) CHECK(conv(2, 3, 3, 0, nullptr, d, 1) == FMPNP_EINVAL);
    CHECK(conv(0, 3, 3, 0, nullptr, 2, 1) == FMPNP_EINVAL);
    CHECK(conv(2, 0, 3, 0, nullptr, 2, 1) == FMPNP_EINVAL);
    CHECK(conv(2, 3, 3, 4, nullptr, 2, 1) == FMPNP_EINVAL);  // an unknown flag
    CHECK(conv(2, 3, 3, FMPNP_CONV_BIAS, nullptr, 2, 1) == FMPNP_EINVAL);
    CHECK(conv(2, 3, 3, 0, nullptr, 2, -1) == FMPNP_EINVAL);
    CHECK(conv(1, 65536, 32768, 0, nullptr, 2, 1) == FMPNP_ETOOBIG);
    CHECK(fmpnp_conv3x3_dilated_cpu(nullptr, 1, 2, 3, 3, w.data(), nullptr, 1, 0, out.data(), 2, 1) == FMPNP_EINVAL);

    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 1, 2, 3, 3, out.data(), 1) == 0);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 1, 2, 1, 9, out.data(), 1) == FMPNP_EINVAL);  // an empty output
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 1, 2, 9, 1, out.data(), 1) == FMPNP_EINVAL);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 0, 2, 3, 3, out.data(), 1) == FMPNP_EINVAL);
    CHECK(fmpnp_avgpool2x2s1_cpu(nullptr, 1, 2, 3, 3, out.data(), 1) == FMPNP_EINVAL);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 1, 2, 3, 3, nullptr, 1) == FMPNP_EINVAL);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 1, 2, 3, 3, out.data(), -1) == FMPNP_EINVAL);
    CHECK(fmpnp_avgpool2x2s1_cpu(in.data(), 1, 1, 65536, 32768, out.data(), 1) == FMPNP_ETOOBIG);

    auto step = [&](const float *c, const float *p, int B, int C, int h, int ww, int hp, int wp, float *o, int f, int t) {
        return fmpnp_dense_pyramid_step_cpu(c, p, B, C, h, ww, hp, wp, o, f, t);
    };
    CHECK(step(in.data(), w.data(), 1, 2, 3, 3, 3, 3, out.data(), 1, 1) == 0);
    CHECK(step(in.data(), nullptr, 1, 2, 3, 3, 0, 0, out.data(), 0, 1) == 0);  // (no prev: its size is ignored)
    CHECK(step(nullptr, nullptr, 1, 2, 3, 3, 0, 0, out.data(), 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), nullptr, 1, 2, 3, 3, 0, 0, nullptr, 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), w.data(), 1, 2, 3, 3, 0, 3, out.data(), 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), w.data(), 1, 2, 3, 3, 3, -1, out.data(), 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), nullptr, 0, 2, 3, 3, 0, 0, out.data(), 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), nullptr, 1, 0, 3, 3, 0, 0, out.data(), 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), nullptr, 1, 2, 0, 3, 0, 0, out.data(), 0, 1) == FMPNP_EINVAL);
    CHECK(step(in.data(), nullptr, 1, 2, 3, 3, 0, 0, out.data(), 2, 1) == FMPNP_EINVAL);  // an unknown flag
    CHECK(step(in.data(), nullptr, 1, 2, 3, 3, 0, 0, out.data(), 0, -1) == FMPNP_EINVAL);
    CHECK(step(in.data(), nullptr, 1, 2, (1 << 24) + 1, 3, 0, 0, out.data(), 0, 1) == FMPNP_ETOOBIG);
    CHECK(step(in.data(), nullptr, 1, 1 << 10, 1 << 11, 1 << 10, 0, 0, out.data(), 0, 1) == FMPNP_ETOOBIG);  // 2^31
    CHECK(step(in.data(), w.data(), 1, 1 << 10, 3, 3, 1 << 11, 1 << 10, out.data(), 0, 1) == FMPNP_ETOOBIG);   // prev
}

}  // namespace

int main() {
    const int shapes[][5] = {{1, 1, 1, 1, 1},  {1, 3, 5, 2, 3},   {2, 5, 64, 7, 9}, {1, 4, 65, 5, 130},
                             {1, 9, 33, 19, 17}, {1, 6, 40, 3, 70}};
    for (const auto &s : shapes)
        for (int d = 1; d <= 2; ++d) {
            conv_shape(s[0], s[1], s[2], s[3], s[4], d, false);
            conv_shape(s[0], s[1], s[2], s[3], s[4], d, true);
        }
    const int pools[][4] = {{1, 1, 2, 2}, {2, 3, 5, 7}, {1, 4, 9, 260}, {1, 2, 2, 300}};
    for (const auto &s : pools) {
        pool_shape(s[0], s[1], s[2], s[3], false);
        pool_shape(s[0], s[1], s[2], s[3], true);
    }
    const int pairs[][4] = {{5, 9, 3, 5}, {4, 7, 9, 13}, {1, 1, 3, 3}, {6, 6, 6, 6}};
    for (int C : {1, 64, 65, 130})
        for (const auto &p : pairs)
            for (int norm = 0; norm < 2; ++norm) {
                step_shape(C == 65 ? 2 : 1, C, p[0], p[1], p[2], p[3], true, norm != 0, false);
                step_shape(1, C, p[0], p[1], p[2], p[3], false, norm != 0, false);
            }
    step_shape(1, 65, 5, 9, 3, 5, true, true, true);
    step_shape(1, 3, 2, 2, 1, 1, false, true, true);
    errors();
    printf(fails ? "test_dense_cpu: %d check(s) FAILED\n" : "test_dense_cpu: all checks passed\n", fails);
    return fails ? 1 : 0;
}
