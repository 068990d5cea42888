// fmpnp_match_layers_impl.h -- the arithmetic of layered matching (include/fmpnp.h, "layered matching"), shared
// by combine_kernel of fmpnp_match_layers.hip and the CPU twin of fmpnp_match_layers_cpu.cpp: both form every
// score with the functions below, which call the taps, the bilerp and the division of fmpnp_hypercolumn_impl.h,
// and neither unit is compiled with contraction, so the two agree bit for bit.  Plain C++ (the twin is built by
// the host compiler), __host__ __device__ under hipcc.
#pragma once
#include "fmpnp_hypercolumn_impl.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fmpnp {
namespace ml {

// one layer's four taps at one output texel, as offsets into a coarse map [H_l][W_l], and their weights
struct Taps {
    int o00, o01, o10, o11;
    float w0x, w1x, w0y, w1y;
};

FMPNP_HC_HD Taps taps_at(int Hl, int Wl, int H, int W, int y, int x) {
    const hc::Tap ty = hc::axis_tap(hc::axis_scale(Hl, H), Hl, y);
    const hc::Tap tx = hc::axis_tap(hc::axis_scale(Wl, W), Wl, x);
    Taps t;
    t.o00 = ty.i0 * Wl + tx.i0;
    t.o01 = ty.i0 * Wl + tx.i1;
    t.o10 = ty.i1 * Wl + tx.i0;
    t.o11 = ty.i1 * Wl + tx.i1;
    t.w0x = tx.w0;
    t.w1x = tx.w1;
    t.w0y = ty.w0;
    t.w1y = ty.w1;
    return t;
}

// r_l: the resize of a row's coarse map at the texel
FMPNP_HC_HD float resized(const float *coarse, const Taps &t) {
    return hc::bilerp(coarse[t.o00], coarse[t.o01], coarse[t.o10], coarse[t.o11], t.w0x, t.w1x, t.w0y, t.w1y);
}

// t = r_0, then t = t + r_l: each add its own fp32 rounding
FMPNP_HC_HD float summed(float t, float r, bool first) { return first ? r : t + r; }

// the columns a correlation launch can index (fmpnp_match.hip dense_match_args)
constexpr long long MAX_WH = (long long)INT32_MAX - (1 << 16);

// argument check shared by the HIP entry points and the twin (host side); *C_out = the channel total,
// *coarse_out = sum_l H_l * W_l, the floats of one row's coarse maps
inline int check_args(const void *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L, int B, int item,
                      int H, int W, int flags, long long *C_out, long long *coarse_out) {
    if (N < 0 || (flags & ~FMPNP_HC_NORMALIZE)) return FMPNP_EINVAL;
    const float probe = 0.0f;  // (hc::check_args wants a dense output; there is none here)
    const int rc = hc::check_args(layers, L, B, &probe, H, W, 0, 0, W, flags, C_out);
    if (rc) return rc;
    if (item < 0 || item >= B || ld_sparse < *C_out) return FMPNP_EINVAL;
    long long coarse = 0;
    for (int l = 0; l < L; ++l) {  // a layer is the correlation's dense operand [C_l][H_l * W_l], ld = stride_c
        const fmpnp_hc_layer &y = layers[l];
        const long long wh = (long long)y.H * y.W;
        if (y.stride_y != y.W || y.stride_c < wh) return FMPNP_EINVAL;
        if (wh > MAX_WH || y.stride_c > INT32_MAX) return FMPNP_ETOOBIG;
        coarse += wh;
    }
    if ((long long)H * W > MAX_WH) return FMPNP_ETOOBIG;
    if (N > 0 && !sparse) return FMPNP_EINVAL;
    *coarse_out = coarse;
    return 0;
}

}  // namespace ml
}  // namespace fmpnp
