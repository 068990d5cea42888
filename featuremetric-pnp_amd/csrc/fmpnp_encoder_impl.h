// fmpnp_encoder_impl.h -- what the encoder's kernels (fmpnp_encoder.hip, fmpnp_conv1x1.hip) and their CPU twins
// (fmpnp_encoder_cpu.cpp, fmpnp_conv1x1_cpu.cpp) share: the argument checks, the ReLU and max-pool expressions and the epilogue of the
// convolution (include/fmpnp.h states the contract).  Plain C++ (the twin is built by the host compiler),
// __host__ __device__ under hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fmpnp.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FMPNP_ENC_HD __host__ __device__ inline
#else
#define FMPNP_ENC_HD inline
#endif

namespace fmpnp {
namespace enc {

// a NaN stays, -0 and everything negative become +0
FMPNP_ENC_HD float relu(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }

// the running maximum of a pool window: a NaN wins, of +0 and -0 the first met stays
FMPNP_ENC_HD float pool_step(float m, float v) { return (v > m || v != v) ? v : m; }
FMPNP_ENC_HD float pool4(float v00, float v01, float v10, float v11) {
    return pool_step(pool_step(pool_step(v00, v01), v10), v11);
}

// the 2 x 2 / stride 1 average (fmpnp_avgpool2x2s1): three fp32 adds in this order, then one multiplication
FMPNP_ENC_HD float avg4(float v00, float v01, float v10, float v11) { return (((v00 + v01) + v10) + v11) * 0.25f; }

// the convolution's epilogue on a finished chain: one fp32 add of the bias, then the ReLU
FMPNP_ENC_HD float finish(float acc, bool has_bias, float bias, bool do_relu) {
    if (has_bias) acc = acc + bias;
    return do_relu ? relu(acc) : acc;
}

constexpr size_t MAX_ELEMS = (size_t)1 << 31;  // every tensor stays below this (32-bit element offsets)

// taps: the weights per input channel, 9 for the 3x3 convolution and 1 for the 1x1 (fmpnp_conv1x1.hip)
inline int conv_args(const void *in, int B, int Cin, int H, int W, const void *weight, const void *bias, int Cout,
                     int flags, const void *out, int taps = 9) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return FMPNP_EINVAL;
    if (flags & ~(FMPNP_CONV_BIAS | FMPNP_CONV_RELU)) return FMPNP_EINVAL;
    const size_t hw = (size_t)H * (size_t)W;  // (< 2^62)
    if (hw >= MAX_ELEMS) return FMPNP_ETOOBIG;
    // (each product below has a factor < 2^31 and a running value < 2^31 once checked: no size_t overflow)
    if ((size_t)B * (size_t)Cin >= MAX_ELEMS || (size_t)B * (size_t)Cin * hw >= MAX_ELEMS) return FMPNP_ETOOBIG;
    if ((size_t)B * (size_t)Cout >= MAX_ELEMS || (size_t)B * (size_t)Cout * hw >= MAX_ELEMS) return FMPNP_ETOOBIG;
    if ((size_t)Cout * (size_t)Cin * (size_t)taps >= MAX_ELEMS) return FMPNP_ETOOBIG;
    if (!in || !weight || !out || ((flags & FMPNP_CONV_BIAS) && !bias)) return FMPNP_EINVAL;
    return 0;
}

// fmpnp_conv3x3_dilated*: the 3x3 convolution's checks, then the dilations built
inline int conv_dilated_args(const void *in, int B, int Cin, int H, int W, const void *weight, const void *bias, int Cout,
                             int flags, const void *out, int dilation) {
    if (dilation != 1 && dilation != 2) return FMPNP_EINVAL;
    return conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out);
}

inline int relu_args(const void *in, const void *out, long long n) {
    if (n < 0) return FMPNP_EINVAL;
    if ((unsigned long long)n >= MAX_ELEMS) return FMPNP_ETOOBIG;
    if (n > 0 && (!in || !out)) return FMPNP_EINVAL;
    return 0;
}

inline int pool_args(const void *in, int B, int C, int H, int W, const void *out) {
    if (B <= 0 || C <= 0 || H < 2 || W < 2) return FMPNP_EINVAL;  // (H or W of 1: an empty output)
    const size_t hw = (size_t)H * (size_t)W;
    if (hw >= MAX_ELEMS || (size_t)B * (size_t)C >= MAX_ELEMS || (size_t)B * (size_t)C * hw >= MAX_ELEMS)
        return FMPNP_ETOOBIG;
    if (!in || !out) return FMPNP_EINVAL;
    return 0;
}

// ---- the fp16 precision (include/fmpnp.h, "the encoder's fp16 precision") ----
// the packed weight image [f16_rows(Cout)][f16_cb(Cin)][9][16] of binary16 values
inline int f16_cb(int Cin) { return (int)(((long long)Cin + 15) / 16); }
inline int f16_rows(int Cout) { return (int)(((long long)Cout + 31) / 32 * 32); }
// its elements, or 0 for an invalid or too large shape (the fp32 weights and the image both stay below 2^31)
inline size_t f16_weight_elems(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0 || (size_t)Cout * (size_t)Cin * 9 >= MAX_ELEMS) return 0;
    const size_t n = ((size_t)Cout + 31) / 32 * 32 * (size_t)f16_cb(Cin) * 9 * 16;
    return n >= MAX_ELEMS ? 0 : n;
}

inline int pack_f16_args(const void *weight, int Cin, int Cout, const void *packed) {
    if (Cin <= 0 || Cout <= 0) return FMPNP_EINVAL;
    if (f16_weight_elems(Cin, Cout) == 0) return FMPNP_ETOOBIG;
    if (!weight || !packed || ((uintptr_t)packed & 15)) return FMPNP_EINVAL;
    return 0;
}

inline int conv_f16_args(const void *in, int B, int Cin, int H, int W, const void *packed, const void *bias, int Cout,
                         int flags, const void *out) {
    const int rc = conv_args(in, B, Cin, H, W, packed, bias, Cout, flags, out);
    if (rc) return rc;
    if (f16_weight_elems(Cin, Cout) == 0) return FMPNP_ETOOBIG;
    return ((uintptr_t)packed & 15) ? FMPNP_EINVAL : 0;
}

}  // namespace enc
}  // namespace fmpnp
