// fmpnp_image_cpu.cpp -- the CPU twins of the image front end (include/fmpnp.h, "image front end"), with HOST
// pointers: fmpnp_image_resize_u8_cpu and fmpnp_image_to_tensor_cpu (fmpnp_image.hip).
//
// The passes consume the tables of img::build_table, which the GPU entry points upload as they are, and form every
// value with the functions of fmpnp_image_impl.h the kernels are built from: integer taps, the shift and the clamp,
// and the value transforms with their true fp32 divisions (this unit is compiled without contraction).  So every
// output byte and float is the GPU's bit for bit, for any n_threads.  Explicit CPU entry points -- parity bridges and
// baselines -- never a fallback of the HIP entry points.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_image_impl.h"

using namespace fmpnp;

namespace {

struct Table {
    std::vector<int32_t> words;
    int ksize = 0, n_out = 0;
    void build(int n_in, int n_out_) {
        n_out = n_out_;
        ksize = img::ksize_of(n_in, n_out);
        words.resize(img::table_words(n_in, n_out));
        std::vector<double> w((size_t)ksize);
        img::build_table(n_in, n_out, words.data(), w.data());
    }
    const int32_t *bounds(int xx) const { return words.data() + 2 * (size_t)xx; }
    const int32_t *k(int xx) const { return words.data() + 2 * (size_t)n_out + (size_t)xx * (size_t)ksize; }
};

// src rows of W pixels -> dst rows of w pixels, `rows` of them
bool horizontal(const uint8_t *src, long long image_stride, long long row_stride, int B, int H, const Table &t, int w,
                uint8_t *dst, int n_threads) {
    return host::deal((long long)B * H, n_threads, [&]() {
        return [=, &t](long long r) {
            const uint8_t *s = src + (r / H) * image_stride + (r % H) * row_stride;
            uint8_t *d = dst + (size_t)r * (size_t)w * 3;
            for (int xx = 0; xx < w; ++xx) {
                const int xmin = t.bounds(xx)[0], xmax = t.bounds(xx)[1];
                const int32_t *k = t.k(xx);
                int a0 = img::ROUND, a1 = img::ROUND, a2 = img::ROUND;
                for (int x = 0; x < xmax; ++x) {
                    const uint8_t *p = s + 3 * (size_t)(xmin + x);
                    a0 = img::tap(a0, p[0], k[x]);
                    a1 = img::tap(a1, p[1], k[x]);
                    a2 = img::tap(a2, p[2], k[x]);
                }
                d[3 * xx] = (uint8_t)img::finish(a0);
                d[3 * xx + 1] = (uint8_t)img::finish(a1);
                d[3 * xx + 2] = (uint8_t)img::finish(a2);
            }
        };
    }, 8);
}

// src images of H rows of n bytes -> dst images of h rows of n bytes
bool vertical(const uint8_t *src, long long image_stride, long long row_stride, int B, const Table &t, int h, int n,
              uint8_t *dst, int n_threads) {
    return host::deal((long long)B * h, n_threads, [&]() {
        return [=, &t, acc = std::vector<int>((size_t)n)](long long r) mutable {
            const int yy = (int)(r % h);
            const int ymin = t.bounds(yy)[0], ymax = t.bounds(yy)[1];
            const int32_t *k = t.k(yy);
            const uint8_t *s = src + (r / h) * image_stride + (long long)ymin * row_stride;
            for (int j = 0; j < n; ++j) acc[(size_t)j] = img::ROUND;
            for (int y = 0; y < ymax; ++y, s += row_stride)
                for (int j = 0; j < n; ++j) acc[(size_t)j] = img::tap(acc[(size_t)j], s[j], k[y]);
            uint8_t *d = dst + (size_t)r * (size_t)n;
            for (int j = 0; j < n; ++j) d[j] = (uint8_t)img::finish(acc[(size_t)j]);
        };
    }, 8);
}

// the resized bytes, contiguous [B][h][w][3] at dst; FMPNP_ENOMEM or 0
int resize(const uint8_t *src, long long image_stride, long long row_stride, int B, int H, int W, int h, int w,
           uint8_t *dst, int n_threads) {
    Table tx, ty;
    std::vector<uint8_t> mid;
    const uint8_t *vsrc = src;
    long long v_is = image_stride, v_rs = row_stride;
    if (w != W) {
        tx.build(W, w);
        uint8_t *hd = dst;
        if (h != H) {
            mid.resize((size_t)B * (size_t)H * (size_t)w * 3);
            hd = mid.data();
            vsrc = hd;
            v_rs = 3LL * w;
            v_is = v_rs * H;
        }
        if (!horizontal(src, image_stride, row_stride, B, H, tx, w, hd, n_threads)) return FMPNP_ENOMEM;
    }
    if (h != H) {
        ty.build(H, h);
        if (!vertical(vsrc, v_is, v_rs, B, ty, h, 3 * w, dst, n_threads)) return FMPNP_ENOMEM;
    } else if (w == W) {
        for (long long r = 0; r < (long long)B * H; ++r)
            memcpy(dst + (size_t)r * (size_t)W * 3, src + (r / H) * image_stride + (r % H) * row_stride, (size_t)W * 3);
    }
    return 0;
}

}  // namespace

extern "C" int fmpnp_image_resize_u8_cpu(const unsigned char *src, long long image_stride, long long row_stride, int B,
                                         int H, int W, int h, int w, unsigned char *dst, int n_threads) {
    const int rc = img::check_args(src, image_stride, row_stride, B, H, W, h, w, dst, 1, 3);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        return resize(src, B > 1 ? image_stride : 0, row_stride, B, H, W, h, w, dst, n_threads);
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}

extern "C" int fmpnp_image_to_tensor_cpu(const unsigned char *src, long long image_stride, long long row_stride, int B,
                                         int H, int W, int h, int w, int mode, int flags, const float *mean,
                                         const float *stdv, float *dst, int n_threads) {
    img::Transform t;
    int rc = img::make_transform(mode, flags, mean, stdv, &t);
    if (rc) return rc;
    rc = img::check_args(src, image_stride, row_stride, B, H, W, h, w, dst, 4, t.channels);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    if (B == 1) image_stride = 0;
    try {
        std::vector<uint8_t> bytes;
        if (h != H || w != W) {
            bytes.resize((size_t)B * (size_t)h * (size_t)w * 3);
            rc = resize(src, image_stride, row_stride, B, H, W, h, w, bytes.data(), n_threads);
            if (rc) return rc;
            src = bytes.data();
            row_stride = 3LL * w;
            image_stride = row_stride * h;
        }
        float lut[3][256];
        for (int c = 0; c < t.channels; ++c)
            for (int p = 0; p < 256; ++p) lut[c][p] = img::value_of(t.kind, p, t.mean[c], t.stdv[c]);
        const size_t plane = (size_t)h * (size_t)w;
        const bool ok = host::deal((long long)B * h, n_threads, [&]() {
            return [=, &lut](long long r) {
                const int b = (int)(r / h), y = (int)(r % h);
                const uint8_t *s = src + b * image_stride + y * row_stride;
                float *d = dst + (size_t)b * (size_t)t.channels * plane + (size_t)y * (size_t)w;
                if (t.gray) {
                    for (int x = 0; x < w; ++x)
                        d[x] = lut[0][img::gray_of(s[3 * x + t.src_c[0]], s[3 * x + 1], s[3 * x + t.src_c[2]])];
                } else {
                    for (int c = 0; c < 3; ++c)
                        for (int x = 0; x < w; ++x) d[(size_t)c * plane + (size_t)x] = lut[c][s[3 * x + t.src_c[c]]];
                }
            };
        }, 8);
        return ok ? 0 : FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}
