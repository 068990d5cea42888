// test_image_cpu.cpp -- the image front end's CPU twins (fmpnp_image_cpu.cpp) against a plain restatement of the
// contract of include/fmpnp.h ("image front end"), stand-alone: no Python, no GPU.  Every output lies between guard
// bytes, the source is a crop view of a larger buffer (row and image strides beyond the image), and the shapes are the
// tests' tiny ones.  `make image-sanitize` builds and runs it under ASan + UBSan; the CPU tests run the plain build.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            ++failures;                      \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);             \
            printf("\n");                    \
        }                                    \
    } while (0)

uint32_t rng_state = 12345u;
uint32_t rng() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// ---- the restatement: one axis at a time over an [n_img][rows][cols][3] image ----
double sinc(double x) { return x == 0.0 ? 1.0 : sin(x * 3.14159265358979323846) / (x * 3.14159265358979323846); }
double lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

// out[i][xx] along an axis of `in` samples; get(i, x) reads, put(i, xx, v) writes; n_lines independent lines
template <class Get, class Put>
void resample(int n_in, int n_out, long long n_lines, Get get, Put put) {
    const double scale = (double)n_in / n_out, fs = scale < 1.0 ? 1.0 : scale, support = 3.0 * fs, ss = 1.0 / fs;
    std::vector<double> w;
    std::vector<long long> k;
    for (int xx = 0; xx < n_out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        w.assign((size_t)xmax, 0.0);
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) ww += w[(size_t)x] = lanczos((x + xmin - center + 0.5) * ss);
        k.assign((size_t)xmax, 0);
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[(size_t)x] / ww : w[(size_t)x];
            k[(size_t)x] = (long long)(v < 0 ? -0.5 + v * 4194304.0 : 0.5 + v * 4194304.0);
        }
        for (long long i = 0; i < n_lines; ++i) {
            long long acc = 1 << 21;
            for (int x = 0; x < xmax; ++x) acc += (long long)get(i, xmin + x) * k[(size_t)x];
            // (floor division by 2^22: the arithmetic shift)
            long long v = acc >= 0 ? acc / 4194304 : -((-acc + 4194303) / 4194304);
            put(i, xx, (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v));
        }
    }
}

// src contiguous [B][H][W][3] -> [B][h][w][3]
std::vector<uint8_t> restated_resize(const std::vector<uint8_t> &src, int B, int H, int W, int h, int w) {
    std::vector<uint8_t> mid = src;
    if (w != W) {
        mid.assign((size_t)B * H * w * 3, 0);
        resample(W, w, (long long)B * H * 3,
                 [&](long long i, int x) { return src[(size_t)((i / 3) * W + x) * 3 + (size_t)(i % 3)]; },
                 [&](long long i, int xx, uint8_t v) { mid[(size_t)((i / 3) * w + xx) * 3 + (size_t)(i % 3)] = v; });
    }
    if (h == H) return mid;
    std::vector<uint8_t> out((size_t)B * h * w * 3);
    const long long line = 3LL * w;
    resample(H, h, (long long)B * line,
             [&](long long i, int y) { return mid[(size_t)(((i / line) * H + y) * line + i % line)]; },
             [&](long long i, int yy, uint8_t v) { out[(size_t)(((i / line) * h + yy) * line + i % line)] = v; });
    return out;
}

constexpr int GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xA5;

struct View {  // a [B][H][W][3] crop of a larger buffer
    std::vector<uint8_t> store;
    long long image_stride, row_stride;
    size_t offset;
    const uint8_t *ptr() const { return store.data() + offset; }
};
View crop_of(const std::vector<uint8_t> &img, int B, int H, int W, bool strided) {
    View v;
    const int pad_x = strided ? 5 : 0, pad_y = strided ? 2 : 0;
    v.row_stride = 3LL * (W + 2 * pad_x) + (strided ? 1 : 0);
    v.image_stride = v.row_stride * (H + 2 * pad_y);
    v.offset = (size_t)(pad_y * v.row_stride + 3 * pad_x);
    v.store.assign((size_t)(v.image_stride * B), 0x5A);
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            memcpy(v.store.data() + v.offset + (size_t)(b * v.image_stride + y * v.row_stride),
                   img.data() + ((size_t)b * H + (size_t)y) * W * 3, (size_t)W * 3);
    return v;
}

template <class T>
bool guards_intact(const std::vector<uint8_t> &buf, size_t n) {
    for (int i = 0; i < GUARD; ++i)
        if (buf[(size_t)i] != GUARD_BYTE || buf[GUARD + n * sizeof(T) + (size_t)i] != GUARD_BYTE) return false;
    return true;
}

void one_shape(int B, int H, int W, int h, int w, int kind) {
    std::vector<uint8_t> img((size_t)B * H * W * 3);
    for (size_t i = 0; i < img.size(); ++i) {
        const size_t px = i / 3, x = px % (size_t)W, y = (px / (size_t)W) % (size_t)H;
        if (kind == 0) img[i] = (uint8_t)rng();
        else if (kind == 1) img[i] = (uint8_t)((x * 255) / (size_t)(W > 1 ? W - 1 : 1) / 2 + (y * 255) / (size_t)(H > 1 ? H - 1 : 1) / 2);
        else img[i] = (rng() & 1) ? 255 : 0;
    }
    const std::vector<uint8_t> want = restated_resize(img, B, H, W, h, w);
    const size_t n_out = (size_t)B * h * w * 3;
    for (int strided = 0; strided < 2; ++strided) {
        const View v = crop_of(img, B, H, W, strided != 0);
        for (int nt : {1, 3}) {
            std::vector<uint8_t> buf(n_out + 2 * GUARD, GUARD_BYTE);
            const int rc = fmpnp_image_resize_u8_cpu(v.ptr(), v.image_stride, v.row_stride, B, H, W, h, w,
                                                     buf.data() + GUARD, nt);
            CHECK(rc == 0, "resize %dx%d -> %dx%d rc %d", H, W, h, w, rc);
            CHECK(guards_intact<uint8_t>(buf, n_out), "resize %dx%d -> %dx%d guard", H, W, h, w);
            CHECK(memcmp(buf.data() + GUARD, want.data(), n_out) == 0, "resize %dx%d -> %dx%d kind %d strided %d nt %d",
                  H, W, h, w, kind, strided, nt);
        }
        // the transforms of the resized bytes
        const float mean[3] = {0.5f, 0.25f, 0.125f}, stdv[3] = {0.3f, 0.2f, 0.1f};
        for (int mode = 0; mode < 4; ++mode)
            for (int variant = 0; variant < 2; ++variant) {
                const bool custom = mode == FMPNP_IMAGE_TORCH && variant;
                const int flags = mode == FMPNP_IMAGE_GRAY && variant ? FMPNP_IMAGE_SWAP_RB : 0;
                if (variant && !custom && !flags) continue;
                const int C = mode == FMPNP_IMAGE_GRAY ? 1 : 3;
                const size_t n = (size_t)B * C * h * w;
                std::vector<uint8_t> buf(n * 4 + 2 * GUARD, GUARD_BYTE);
                float *out = (float *)(buf.data() + GUARD);
                const int rc = fmpnp_image_to_tensor_cpu(v.ptr(), v.image_stride, v.row_stride, B, H, W, h, w, mode, flags,
                                                         custom ? mean : nullptr, custom ? stdv : nullptr, out, 2);
                CHECK(rc == 0, "to_tensor mode %d rc %d", mode, rc);
                CHECK(guards_intact<float>(buf, n), "to_tensor mode %d guard", mode);
                size_t bad = 0;
                for (int b = 0; b < B; ++b)
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < w; ++x) {
                            const uint8_t *p = want.data() + (((size_t)b * h + (size_t)y) * w + (size_t)x) * 3;
                            for (int c = 0; c < C; ++c) {
                                volatile float e;
                                if (mode == FMPNP_IMAGE_TORCH) {
                                    static const float tm[3] = {0.485f, 0.456f, 0.406f}, ts[3] = {0.229f, 0.224f, 0.225f};
                                    volatile float u = (float)p[c] / 255.0f;
                                    volatile float d = u - (custom ? mean[c] : tm[c]);
                                    e = d / (custom ? stdv[c] : ts[c]);
                                } else if (mode == FMPNP_IMAGE_CAFFE) {
                                    static const float cm[3] = {103.939f, 116.779f, 123.68f};
                                    e = (float)p[2 - c] - cm[c];
                                } else if (mode == FMPNP_IMAGE_RAW) {
                                    e = (float)p[c];
                                } else {
                                    const int a = flags ? p[2] : p[0], bb = flags ? p[0] : p[2];
                                    e = (float)((9798 * a + 19235 * p[1] + 3735 * bb + 16384) >> 15) / 255.0f;
                                }
                                const float got = out[(((size_t)b * C + (size_t)c) * h + (size_t)y) * w + (size_t)x];
                                const float ev = e;
                                if (memcmp(&got, &ev, 4) != 0) ++bad;
                            }
                        }
                CHECK(bad == 0, "to_tensor %dx%d -> %dx%d mode %d variant %d: %zu values differ", H, W, h, w, mode, variant,
                      bad);
            }
    }
}

void error_paths() {
    std::vector<uint8_t> src(8 * 8 * 3, 1), dst(8 * 8 * 3 * 4);
    float *fd = (float *)dst.data();
    const float m[3] = {0, 0, 0};
    CHECK(fmpnp_image_resize_u8_cpu(nullptr, 0, 24, 1, 8, 8, 4, 4, dst.data(), 1) == FMPNP_EINVAL, "null src");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, nullptr, 1) == FMPNP_EINVAL, "null dst");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 0, 8, 8, 4, 4, dst.data(), 1) == FMPNP_EINVAL, "B = 0");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 1, 8, 8, 0, 4, dst.data(), 1) == FMPNP_EINVAL, "h = 0");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 1, 8, 8, 4, -1, dst.data(), 1) == FMPNP_EINVAL, "w < 0");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 23, 1, 8, 8, 4, 4, dst.data(), 1) == FMPNP_EINVAL, "short row stride");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 90, 24, 2, 4, 8, 4, 4, dst.data(), 1) == FMPNP_EINVAL, "short image stride");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, src.data() + 10, 1) == FMPNP_EINVAL, "overlap");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, dst.data(), -1) == FMPNP_EINVAL, "n_threads < 0");
    CHECK(fmpnp_image_resize_u8_cpu(src.data(), 0, 24, 1, 8, 8, 4, 16385, dst.data(), 1) == FMPNP_ETOOBIG, "w too big");
    CHECK(fmpnp_image_to_tensor_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, 7, 0, nullptr, nullptr, fd, 1) == FMPNP_EINVAL, "mode");
    CHECK(fmpnp_image_to_tensor_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, FMPNP_IMAGE_TORCH, 1, nullptr, nullptr, fd, 1) ==
              FMPNP_EINVAL, "flag without gray");
    CHECK(fmpnp_image_to_tensor_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, FMPNP_IMAGE_GRAY, 2, nullptr, nullptr, fd, 1) ==
              FMPNP_EINVAL, "unknown flag");
    CHECK(fmpnp_image_to_tensor_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, FMPNP_IMAGE_RAW, 0, m, nullptr, fd, 1) ==
              FMPNP_EINVAL, "mean with raw");
    CHECK(fmpnp_image_to_tensor_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, FMPNP_IMAGE_CAFFE, 0, nullptr, m, fd, 1) ==
              FMPNP_EINVAL, "std with caffe");
    CHECK(fmpnp_image_to_tensor_cpu(src.data(), 0, 24, 1, 8, 8, 4, 4, FMPNP_IMAGE_TORCH, 0, nullptr, nullptr, nullptr, 1) ==
              FMPNP_EINVAL, "null float dst");
}

}  // namespace

int main() {
    const int shapes[][4] = {{37, 53, 16, 24}, {37, 53, 37, 20}, {37, 53, 11, 53}, {40, 40, 40, 40}, {23, 31, 64, 80},
                             {7, 5, 3, 2},     {5, 7, 1, 1},     {96, 128, 25, 33}, {128, 96, 16, 12}, {3, 400, 2, 5}};
    for (const auto &s : shapes)
        for (int kind = 0; kind < 3; ++kind) one_shape(kind == 0 ? 2 : 1, s[0], s[1], s[2], s[3], kind);
    error_paths();
    if (failures) {
        printf("test_image_cpu: %d FAILED\n", failures);
        return 1;
    }
    printf("test_image_cpu: OK\n");
    return 0;
}
