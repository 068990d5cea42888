// fmpnp_image_impl.h -- what the image front end's kernels (fmpnp_image.hip) and their CPU twins
// (fmpnp_image_cpu.cpp) share: the coefficient tables of Pillow's 8-bit Lanczos resampling, one tap and the rounding of
// a pass, the value transforms, and the argument checks (include/fmpnp.h, "image front end", states the contract).
// Plain C++ (the twin is built by the host compiler), __host__ __device__ under hipcc; neither unit is compiled with
// contraction.  The tables are built on the host only, in double with the C library's sin, and both sides consume the
// same table.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fmpnp.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FMPNP_IMG_HD __host__ __device__ inline
#else
#define FMPNP_IMG_HD inline
#endif

namespace fmpnp {
namespace img {

constexpr int MAX_DIM = 16384;       // every image size, source and output
constexpr int PRECISION_BITS = 22;   // Pillow's 32 - 8 - 2
constexpr int ROUND = 1 << (PRECISION_BITS - 1);
// an axis table: int32 bounds[out][2] = (xmin, xmax), then int32 k[out][ksize] (zero behind xmax)
// out * ksize <= 6 max(in, out) + 3 out, so a table has at most 11 MAX_DIM words
constexpr size_t TABLE_MAX_BYTES = (size_t)11 * MAX_DIM * 4;

inline int ksize_of(int n_in, int n_out) {
    double fs = (double)n_in / (double)n_out;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(3.0 * fs) * 2 + 1;
}
inline size_t table_words(int n_in, int n_out) { return (size_t)n_out * (size_t)(ksize_of(n_in, n_out) + 2); }

inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}
inline double lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

// the table of one axis (table_words(n_in, n_out) words at `table`); w: [ksize] doubles of scratch
inline void build_table(int n_in, int n_out, int32_t *table, double *w) {
    const int ksize = ksize_of(n_in, n_out);
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs, ss = 1.0 / fs;  // (Pillow multiplies by 1 / fs; so does this)
    int32_t *bounds = table, *kk = table + 2 * (size_t)n_out;
    for (int xx = 0; xx < n_out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = lanczos((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t *k = kk + (size_t)xx * (size_t)ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (double)(1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// a product of two values that fit 24 signed bits (the device's 24-bit multiplier)
#if defined(__HIP_DEVICE_COMPILE__)
FMPNP_IMG_HD int mul_small(int a, int b) { return __mul24(a, b); }
#else
FMPNP_IMG_HD int mul_small(int a, int b) { return a * b; }
#endif
// one tap of a pass: a pixel (8 bits) times a coefficient (24 signed bits), summed in int32
FMPNP_IMG_HD int tap(int acc, int p, int k) { return acc + mul_small(p, k); }
// a pass's result from its accumulator (which started at ROUND): arithmetic shift, then the clamp
FMPNP_IMG_HD int finish(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// the gray value of three bytes: a weighs 9798, g 19235, b 3735 (of 32768), rounded to nearest
FMPNP_IMG_HD int gray_of(int a, int g, int b) {
    return (mul_small(9798, a) + mul_small(19235, g) + mul_small(3735, b) + 16384) >> 15;
}

// the float of byte p in output channel c: kinds of the value table
enum { LUT_TORCH = 0, LUT_SUB = 1, LUT_UNIT = 2 };
FMPNP_IMG_HD float value_of(int kind, int p, float mean, float stdv) {
    const float f = (float)p;
    if (kind == LUT_SUB) return f - mean;
    const float u = f / 255.0f;
    if (kind == LUT_UNIT) return u;
    const float d = u - mean;
    return d / stdv;
}

// what a call's mode resolves to: the table kind, the output's channel count, and for output channel c the source
// channel src_c[c]; gray: (a, g, b) = source channels (src_c[0], 1, src_c[2])
struct Transform {
    int kind, channels, gray;
    int src_c[3];
    float mean[3], stdv[3];
};
inline int make_transform(int mode, int flags, const float *mean, const float *stdv, Transform *t) {
    if (flags & ~FMPNP_IMAGE_SWAP_RB) return FMPNP_EINVAL;
    static const float tm[3] = {0.485f, 0.456f, 0.406f}, ts[3] = {0.229f, 0.224f, 0.225f};
    static const float cm[3] = {103.939f, 116.779f, 123.68f};
    Transform r = {};
    r.channels = 3;
    for (int c = 0; c < 3; ++c) {
        r.src_c[c] = c;
        r.mean[c] = 0.f;
        r.stdv[c] = 1.f;
    }
    switch (mode) {
    case FMPNP_IMAGE_TORCH:
        r.kind = LUT_TORCH;
        for (int c = 0; c < 3; ++c) {
            r.mean[c] = mean ? mean[c] : tm[c];
            r.stdv[c] = stdv ? stdv[c] : ts[c];
        }
        break;
    case FMPNP_IMAGE_CAFFE:
        r.kind = LUT_SUB;
        for (int c = 0; c < 3; ++c) {
            r.src_c[c] = 2 - c;
            r.mean[c] = mean ? mean[c] : cm[c];
        }
        if (stdv) return FMPNP_EINVAL;
        break;
    case FMPNP_IMAGE_RAW:
        r.kind = LUT_SUB;  // (p - 0 is p)
        if (mean || stdv) return FMPNP_EINVAL;
        break;
    case FMPNP_IMAGE_GRAY:
        r.kind = LUT_UNIT;
        r.channels = 1;
        r.gray = 1;
        if (mean || stdv) return FMPNP_EINVAL;
        if (flags & FMPNP_IMAGE_SWAP_RB) {
            r.src_c[0] = 2;
            r.src_c[2] = 0;
        }
        break;
    default:
        return FMPNP_EINVAL;
    }
    if (mode != FMPNP_IMAGE_GRAY && flags) return FMPNP_EINVAL;
    *t = r;
    return 0;
}

// argument check of every entry point (host side).  dst_bytes: the destination's size; strides in bytes
inline int check_args(const void *src, long long image_stride, long long row_stride, int B, int H, int W, int h, int w,
                      const void *dst, size_t dst_elem, int dst_channels) {
    if (!src || !dst || B < 1 || H < 1 || W < 1 || h < 1 || w < 1) return FMPNP_EINVAL;
    if (H > MAX_DIM || W > MAX_DIM || h > MAX_DIM || w > MAX_DIM || B > MAX_DIM) return FMPNP_ETOOBIG;
    if (row_stride < 3LL * W) return FMPNP_EINVAL;
    if (B > 1 && image_stride < (long long)(H - 1) * row_stride + 3LL * W) return FMPNP_EINVAL;
    if (row_stride > ((long long)1 << 40) || image_stride > ((long long)1 << 40)) return FMPNP_ETOOBIG;
    const unsigned long long s0 = (unsigned long long)(uintptr_t)src;
    const unsigned long long s1 =
        s0 + (unsigned long long)(B - 1) * (unsigned long long)(B > 1 ? image_stride : 0) +
        (unsigned long long)(H - 1) * (unsigned long long)row_stride + 3ULL * (unsigned long long)W;
    const unsigned long long d0 = (unsigned long long)(uintptr_t)dst;
    const unsigned long long d1 = d0 + (unsigned long long)B * (unsigned long long)dst_channels * (unsigned long long)h *
                                           (unsigned long long)w * (unsigned long long)dst_elem;
    if (d1 - d0 >= (1ULL << 33)) return FMPNP_ETOOBIG;
    if (s0 < d1 && d0 < s1) return FMPNP_EINVAL;  // (the destination overlaps the source)
    return 0;
}

}  // namespace img
}  // namespace fmpnp
