// fmpnp_retrieval_impl.h -- the arithmetic of the retrieval stage (include/fmpnp.h states the contract),
// shared by the kernels of fmpnp_retrieval.hip and the CPU twin of fmpnp_retrieval_cpu.cpp: both call
// these functions for every value they form outside the fmaf chains of the products, and neither unit is
// compiled with contraction, so the two agree bit for bit.  Plain C++ (the twin is built by the host
// compiler), __host__ __device__ under hipcc.  Neither side calls a library exp: exp_neg below is the
// only exponential, built from fmaf and integer exponent assembly.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "fmpnp.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FMPNP_RV_HD __host__ __device__ inline
#else
#define FMPNP_RV_HD inline
#endif

namespace fmpnp {
namespace rv {

constexpr int SEG = FMPNP_NETVLAD_SEGMENT;  // positions per aggregation segment: part of the contract
constexpr int NORM_CHAINS = 4;              // interleaved chains of an input position's sum of squares
constexpr int ROW_CHAINS = 64;              // interleaved chains of a cluster row's sums of squares
constexpr int RANK_CAP = FMPNP_RANK_TOPN_CAP;
constexpr int MAX_SIZE = 1 << 24;           // K, C, P, B, Q, R, D

FMPNP_RV_HD float bits_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
FMPNP_RV_HD uint32_t float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}

// exp(x) for x <= 0 (NaN in, NaN out; below -104.5, -Inf included: +0).  n = round(x log2 e) by the
// 1.5 * 2^23 shift, r = x - n ln 2 in two fmaf steps (the high part of ln 2 has 9 bits: n * hi is exact),
// exp(r) = 1 + r + r^2 P(r) by Horner in fmaf, and 2^n assembled in the exponent field -- through
// 2^(n + 64) * 2^-64 below the normal range, so a subnormal result is rounded once.  Measured against the
// correctly rounded exponential over every float in [-104, 0]: FMPNP_NETVLAD_EXP_MAX_ULP (include/fmpnp.h).
FMPNP_RV_HD float exp_neg(float x) {
    if (!(x >= -104.5f)) return x != x ? x : 0.0f;
    const float shift = 12582912.0f;  // 1.5 * 2^23
    const float t = __builtin_fmaf(x, 1.44269504088896341f, shift);
    const float nf = t - shift;
    const int n = (int)(float_bits(t) - 0x4b400000u);  // (the integer in t's low mantissa bits, two's complement)
    float r = __builtin_fmaf(nf, -0.693359375f, x);
    r = __builtin_fmaf(nf, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, r * r, r) + 1.0f;
    if (n >= -126) return y * bits_float((uint32_t)(n + 127) << 23);
    return (y * bits_float((uint32_t)(n + 64 + 127) << 23)) * 5.42101086242752217e-20f;  // 2^-64
}

// one link of a chain of squares
FMPNP_RV_HD float square_link(float v, float acc) { return __builtin_fmaf(v, v, acc); }

// max(sqrt(sum), 1e-12): F.normalize's denominator
FMPNP_RV_HD float norm_floor(float sum) {
    const float n = __builtin_sqrtf(sum);
    return n > 1e-12f ? n : (n != n ? n : 1e-12f);
}

// an input position's denominator from its NORM_CHAINS partial sums of squares
FMPNP_RV_HD float position_norm(float s0, float s1, float s2, float s3) { return norm_floor((s0 + s1) + (s2 + s3)); }

FMPNP_RV_HD float quotient(float v, float n) { return v / n; }

// the maximum that ignores NaN (NaN only when both are): any order of the logits gives the same value
// up to the sign of a zero, which the softmax does not see
FMPNP_RV_HD float max_link(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }

// vlad = V - S * centroid, one rounding
FMPNP_RV_HD float centroid_term(float V, float S, float centroid) { return __builtin_fmaf(-S, centroid, V); }

// The ranking key: greater key = better rank.  NaN is the lowest key (np.argsort(-scores) puts NaN last),
// -0 counts as +0; otherwise the order of the floats.  (The match select's key puts NaN first instead.)
FMPNP_RV_HD uint32_t rank_key(float x) {
    if (x != x) return 0u;
    const uint32_t u = float_bits(x + 0.0f);  // (-0 + +0 = +0)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// key and reference index in one word: greater = ranks earlier (the lower index among equal keys)
FMPNP_RV_HD uint64_t rank_word(float x, uint32_t index) { return ((uint64_t)rank_key(x) << 32) | (uint32_t)~index; }
FMPNP_RV_HD uint32_t word_index(uint64_t w) { return ~(uint32_t)w; }

// argument checks shared by the HIP entry points and the twins (host side)
inline int pool_args(const float *x, int B, int C, int P, long long sb, long long sc, const float *w, int K, int ld_w,
                     const float *cent, int ld_c, int normalize_input, const float *out, long long ld_out) {
    if (B < 0 || K < 1 || C < 1 || P < 1) return FMPNP_EINVAL;
    if (normalize_input != 0 && normalize_input != 1) return FMPNP_EINVAL;
    if (sc < P || sb < 0 || ld_w < C || ld_c < C) return FMPNP_EINVAL;
    if (K > MAX_SIZE || C > MAX_SIZE || P > MAX_SIZE - SEG || B > MAX_SIZE) return FMPNP_ETOOBIG;
    if ((long long)K * (long long)C > (long long)INT32_MAX - 1024) return FMPNP_ETOOBIG;
    if (ld_out < (long long)K * (long long)C) return FMPNP_EINVAL;
    if (B > 0 && (!x || !w || !cent || !out)) return FMPNP_EINVAL;
    return 0;
}

inline int rank_args(const float *qry, int Q, int ld_q, const float *ref_t, int D, int R, int ld_r, int n,
                     const int *idx, const float *top) {
    if (Q < 0 || D < 1 || R < 1 || ld_q < D || ld_r < R || n < 1 || n > R) return FMPNP_EINVAL;
    if (n > RANK_CAP || Q > MAX_SIZE || D > MAX_SIZE || R > MAX_SIZE) return FMPNP_ETOOBIG;
    if (Q > 0 && (!qry || !ref_t || !idx || !top)) return FMPNP_EINVAL;
    return 0;
}

}  // namespace rv
}  // namespace fmpnp
