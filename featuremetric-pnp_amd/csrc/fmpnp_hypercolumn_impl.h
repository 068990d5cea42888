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

// ---- sparse hypercolumns (fmpnp_hypercolumn_sparse*): the texel of a point ------------------------------------
// Each rule is stated once here; the kernel of fmpnp_hypercolumn_sparse.hip and its CPU twin both call locate().

// (int)v as the device's cast gives it, without the host's undefined behaviour: false for a NaN and for a value
// whose truncation is no int (the device's cast would saturate: far outside any map, an error either way)
FMPNP_HC_HD bool to_index(double v, int *i) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return false;
    *i = (int)v;
    return true;
}

// FMPNP_HC_AT_REFERENCE: fmpnp_gather_reference's index (optimize_feature_pnp.py:51-56; the swap of H and W
// between the two factors is the reference's).  A negative index down to -H / -W wraps, as Python's does.
FMPNP_HC_HD bool index_reference(double x, double y, int H, int W, double img0, double img1, int *row, int *col) {
    const double rel0 = (double)H / img0, rel1 = (double)W / img1;
    const double colf = rel0 * x, rowf = rel1 * y;
    int c, r;
    if (!to_index(colf, &c) || !to_index(rowf, &r)) return false;
    if (r < 0 && r >= -H) r += H;
    if (c < 0 && c >= -W) c += W;
    if (r < 0 || r >= H || c < 0 || c >= W) return false;
    *row = r;
    *col = c;
    return true;
}

// FMPNP_HC_AT_CELL: fmpnp_gather_sparse_descriptors' index, the nearest centre of generate_dense_keypoints'
// grid (keypoint_association.py:26-38, 77-86): the lower cell on an exact edge, cell 0 for a NaN
FMPNP_HC_HD int nearest_cell(double p, double cell, int n) {
    const double c = ceil(p / cell - 1.0);
    return c > 0.0 ? (c < (double)(n - 1) ? (int)c : n - 1) : 0;
}

// the (batch item, row, col) of point p, or false: the row is then an error row
FMPNP_HC_HD bool locate(const void *points, const int *item, int p, int at, double p0, double p1, int B, int H, int W,
                        int *b, int *row, int *col) {
    *b = item ? item[p] : 0;
    if (*b < 0 || *b >= B) return false;
    if (at == FMPNP_HC_AT_TEXEL) {
        const int *q = (const int *)points + 2 * (size_t)p;
        *row = q[0];
        *col = q[1];
        return *row >= 0 && *row < H && *col >= 0 && *col < W;
    }
    const double *q = (const double *)points + 2 * (size_t)p;
    if (at == FMPNP_HC_AT_REFERENCE) return index_reference(q[0], q[1], H, W, p0, p1, row, col);
    *col = nearest_cell(q[0], p1, W);  // coordinate 0 runs along the map's last dimension
    *row = nearest_cell(q[1], p0, H);
    return true;
}

// the resized value of channel c (of the layer) of batch item b at the output texel whose taps are ty, tx
FMPNP_HC_HD float value_at(const fmpnp_hc_layer &ly, int b, int c, const Tap &ty, const Tap &tx) {
    const float *plane = ly.data + (size_t)b * (size_t)ly.stride_b + (size_t)c * (size_t)ly.stride_c;
    const float *r0 = plane + (size_t)ty.i0 * (size_t)ly.stride_y, *r1 = plane + (size_t)ty.i1 * (size_t)ly.stride_y;
    return bilerp(r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1], tx.w0, tx.w1, ty.w0, ty.w1);
}

// argument check of the sparse entry points (host side): the layers and sizes as check_args, then the rest
inline int check_sparse_args(const fmpnp_hc_layer *layers, int L, int B, int H, int W, const void *points, int N,
                             int at, double p0, double p1, const void *out, int dtype_out, long long ld_out, int flags,
                             long long *C_out) {
    if (N < 0 || (flags & ~FMPNP_HC_NORMALIZE)) return FMPNP_EINVAL;
    const float probe = 0.0f;  // (check_args wants a dense output; the sparse one is checked below)
    const int rc = check_args(layers, L, B, &probe, H, W, 0, 0, W, flags, C_out);
    if (rc) return rc;
    if (at != FMPNP_HC_AT_TEXEL && at != FMPNP_HC_AT_REFERENCE && at != FMPNP_HC_AT_CELL) return FMPNP_EINVAL;
    if (at != FMPNP_HC_AT_TEXEL && !(p0 > 0.0 && p1 > 0.0)) return FMPNP_EINVAL;  // (a NaN too)
    if (dtype_out != FMPNP_F32 && dtype_out != FMPNP_F64) return FMPNP_EINVAL;
    if (ld_out < *C_out) return FMPNP_EINVAL;
    if (N > 0 && (!points || !out)) return FMPNP_EINVAL;
    return 0;
}

}  // namespace hc
}  // namespace fmpnp
