// fmpnp_hypercolumn_impl.h -- the arithmetic of the hypercolumn assembly (include/fmpnp.h states the
// contract), shared by the kernel of fmpnp_hypercolumn.hip and the CPU twin of fmpnp_hypercolumn_cpu.cpp:
// both call these functions for every value they form, and neither unit is compiled with contraction, so
// the two agree bit for bit.  Plain C++ (the twin is built by the host compiler), __host__ __device__
// under hipcc.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fmpnp.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FMPNP_HC_HD __host__ __device__ inline
#else
#define FMPNP_HC_HD inline
#endif

namespace fmpnp {
namespace hc {

constexpr int BLOCK = 64;      // channels per fp64 partial sum: part of the contract
constexpr int MAX_LAYERS = 8;
constexpr int MAX_SIZE = 1 << 24;  // every size: (float)d is exact and (int)src cannot overflow

// one axis's two taps and their weights at output coordinate d
struct Tap {
    int i0, i1;
    float w0, w1;
};

FMPNP_HC_HD float axis_scale(int n_in, int n_out) {
    return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f;
}

FMPNP_HC_HD Tap axis_tap(float scale, int n_in, int d) {
    const float src = scale * (float)d;
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > n_in - 1) t.i0 = n_in - 1;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.w1 = src - (float)t.i0;
    t.w0 = 1.0f - t.w1;
    return t;
}

// a, b: the values at (y0, x0), (y0, x1); c, d: at (y1, x0), (y1, x1)
FMPNP_HC_HD float bilerp(float a, float b, float c, float d, float w0x, float w1x, float w0y, float w1y) {
    const float top = w0x * a + w1x * b;
    const float bot = w0x * c + w1x * d;
    return w0y * top + w1y * bot;
}

// one link of a block's chain of squares
FMPNP_HC_HD double square_acc(float v, double acc) { return fma((double)v, (double)v, acc); }

FMPNP_HC_HD float norm_of(double sum) { return (float)sqrt(sum); }

FMPNP_HC_HD float normalised(float v, float n) { return v / n; }

// argument check shared by the HIP entry points and the twin (host side)
inline int check_args(const fmpnp_hc_layer *layers, int L, int B, const float *out, int H, int W, long long osb,
                      long long osc, long long osy, int flags, long long *C_out) {
    if (L < 1 || L > MAX_LAYERS || !layers || !out || B < 1 || H < 1 || W < 1) return FMPNP_EINVAL;
    if (flags & ~(FMPNP_HC_NORMALIZE | FMPNP_HC_DWORD_STORES | FMPNP_HC_VECTOR_STORES)) return FMPNP_EINVAL;
    if (osb < 0 || osc < 0 || osy < W) return FMPNP_EINVAL;
    long long C = 0;
    for (int l = 0; l < L; ++l) {
        const fmpnp_hc_layer &y = layers[l];
        if (!y.data || y.C < 1 || y.H < 1 || y.W < 1) return FMPNP_EINVAL;
        if (y.stride_b < 0 || y.stride_c < 0 || y.stride_y < y.W) return FMPNP_EINVAL;
        C += y.C;
    }
    if (H > MAX_SIZE || W > MAX_SIZE || B > MAX_SIZE || C > MAX_SIZE) return FMPNP_ETOOBIG;
    for (int l = 0; l < L; ++l)
        if (layers[l].H > MAX_SIZE || layers[l].W > MAX_SIZE) return FMPNP_ETOOBIG;
    *C_out = C;
    return 0;
}

}  // namespace hc
}  // namespace fmpnp
