// fmpnp_superpoint_impl.h -- the arithmetic and the decisions of the SuperPoint baseline's five stages
// (include/fmpnp.h states the contract), shared by the kernels of fmpnp_superpoint.hip and the CPU twins of
// fmpnp_superpoint_cpu.cpp: both call these functions for every value they form and neither unit is compiled
// with contraction, so the two agree bit for bit.  The units differ only in how they walk the data (tiles,
// waves and ballots on the GPU, loops on the host).  Plain C++ (the twin is built by the host compiler),
// __host__ __device__ under hipcc.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_retrieval_impl.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FMPNP_SP_HD __host__ __device__ inline
#else
#define FMPNP_SP_HD inline
#endif

namespace fmpnp {
namespace sp {

constexpr int CELL = FMPNP_SP_CELL;            // pixels per side of a detector cell
constexpr int DUST = CELL * CELL;              // the dustbin channel
constexpr int MAX_DIST = FMPNP_SP_MAX_NMS_DIST;
constexpr int MAX_SIDE = 1 << 14;              // H, W: H * W and the keep capacity stay below 2^31
constexpr int MAX_COUNT = 1 << 24;             // keypoints, landmarks, channels
constexpr int CHAINS = 64;                     // interleaved chains of a descriptor's sum of squares
enum : unsigned char { EMPTY = 0, LIVE = 1, KEPT = 2, GONE = 3 };

using rv::bits_float;
using rv::float_bits;

// exp(x) for any x: the retrieval stage's routine for x <= 0, and the same reduction, polynomial and
// exponent assembly above 0 (2^n in two exact steps, so the last product rounds or overflows once);
// +Inf from 89 up, NaN in, NaN out.
FMPNP_SP_HD float exp_any(float x) {
    if (!(x > 0.0f)) return rv::exp_neg(x);
    if (x >= 89.0f) return bits_float(0x7f800000u);
    const float shift = 12582912.0f;  // 1.5 * 2^23
    const float t = __builtin_fmaf(x, 1.44269504088896341f, shift);
    const float nf = t - shift;
    const int n = (int)(float_bits(t) - 0x4b400000u);
    float r = __builtin_fmaf(nf, -0.693359375f, x);
    r = __builtin_fmaf(nf, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, r * r, r) + 1.0f;
    const int n1 = n / 2, n2 = n - n1;  // (0 <= n <= 129: both factors are normal)
    return (y * bits_float((uint32_t)(n1 + 127) << 23)) * bits_float((uint32_t)(n2 + 127) << 23);
}

// ---- 1. detector head: one cell's 65 logits -> its 64 heat values (demo_superpoint.py:240-250) ------------
// logit(c) reads channel c of the cell; put(c, v) stores the heat value of channel c < 64
template <class Logit, class Put>
FMPNP_SP_HD void cell_heat(Logit logit, Put put) {
    float e[DUST + 1];
    float s = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c <= DUST; ++c) {
        e[c] = exp_any(logit(c));
        s = c == 0 ? e[0] : s + e[c];
    }
    const float den = s + 1e-5f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < DUST; ++c) put(c, e[c] / den);
}

// ---- 2. NMS: the order of the candidates ------------------------------------------------------------------
FMPNP_SP_HD bool is_candidate(float heat, float thresh) { return heat >= thresh; }  // (NaN: no)
// greater word = earlier in the greedy walk: the confidence, then the lower row-major pixel index
FMPNP_SP_HD uint64_t nms_word(float heat, uint32_t pixel) { return rv::rank_word(heat, pixel); }
FMPNP_SP_HD bool on_border(int x, int y, int W, int H, int border) {
    return x < border || x >= W - border || y < border || y >= H - border;
}
// the most points the NMS can keep: one per (d + 1) x (d + 1) cell
FMPNP_SP_HD long long keep_capacity(int H, int W, int d) {
    return (long long)((H + d) / (d + 1)) * (long long)((W + d) / (d + 1));
}

// ---- 3. descriptor sampling (demo_superpoint.py:273-283, grid_sample's bilinear, zero padding) ------------
FMPNP_SP_HD float grid_coord(double pixel, int size) { return (float)(pixel / ((double)size / 2.) - 1.); }
FMPNP_SP_HD float unnormalize(float g, int size, int align_corners) {
    if (align_corners) return ((g + 1.0f) / 2.0f) * (float)(size - 1);
    return ((g + 1.0f) * (float)size - 1.0f) / 2.0f;
}
struct Taps {
    int x0, y0;        // the north-west tap; the others are at +1
    float w[4];        // nw, ne, sw, se
    bool in[4];
};
FMPNP_SP_HD Taps make_taps(double px, double py, int W, int H, int Wc, int Hc, int align_corners) {
    Taps t;
    const float ix = unnormalize(grid_coord(px, W), Wc, align_corners);
    const float iy = unnormalize(grid_coord(py, H), Hc, align_corners);
    const float fx = __builtin_floorf(ix), fy = __builtin_floorf(iy);
    const float ex = fx + 1.0f, ey = fy + 1.0f;
    t.w[0] = (ex - ix) * (ey - iy);
    t.w[1] = (ix - fx) * (ey - iy);
    t.w[2] = (ex - ix) * (iy - fy);
    t.w[3] = (ix - fx) * (iy - fy);
    // (a coordinate beyond the int range, or NaN, has no tap inside the map)
    const bool fin = fx >= -2.0f && fx <= (float)(1 << 20) && fy >= -2.0f && fy <= (float)(1 << 20);
    t.x0 = fin ? (int)fx : -2;
    t.y0 = fin ? (int)fy : -2;
    for (int k = 0; k < 4; ++k) {
        const int x = t.x0 + (k & 1), y = t.y0 + (k >> 1);
        t.in[k] = x >= 0 && x < Wc && y >= 0 && y < Hc;
    }
    return t;
}
// one channel's sample: the in-bounds taps' products added in the order nw, ne, sw, se from +0
FMPNP_SP_HD float sample(const float *plane, int Wc, const Taps &t) {
    float acc = 0.0f;
    for (int k = 0; k < 4; ++k) {
        if (!t.in[k]) continue;
        const float v = plane[(size_t)(t.y0 + (k >> 1)) * (size_t)Wc + (size_t)(t.x0 + (k & 1))];
        const float prod = v * t.w[k];
        acc = acc + prod;
    }
    return acc;
}
FMPNP_SP_HD float square_link(float v, float acc) { return __builtin_fmaf(v, v, acc); }
FMPNP_SP_HD float desc_norm(float sum) { return __builtin_sqrtf(sum); }

// ---- 4. two nearest neighbours ----------------------------------------------------------------------------
FMPNP_SP_HD float score_dist(float s) {
    const float one = 1.0f - s;
    return 2.0f * one;
}
// ascending order of the distances: NaN after every number, -0 counts as +0
FMPNP_SP_HD uint32_t dist_key(float d) {
    if (d != d) return 0xffffffffu;
    const uint32_t u = float_bits(d + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// smaller word = nearer; the lower index among equal distances
FMPNP_SP_HD uint64_t dist_word(float d, uint32_t index) { return ((uint64_t)dist_key(d) << 32) | index; }
constexpr uint64_t NO_WORD = ~(uint64_t)0;
// (a, b) sorted, a < b or both NO_WORD: take w in
FMPNP_SP_HD void two_insert(uint64_t &a, uint64_t &b, uint64_t w) {
    if (w < a) {
        b = a;
        a = w;
    } else if (w < b) {
        b = w;
    }
}
FMPNP_SP_HD float ratio_squared(double ratio) { return (float)(ratio * ratio); }
FMPNP_SP_HD bool ratio_ok(float d0, float d1, float ratio2) {
    const float bound = ratio2 * d1;
    return d0 <= bound;
}

// ---- 5. landmark association ------------------------------------------------------------------------------
FMPNP_SP_HD double landmark_dist(double px, double py, double rx, double ry) {
    const double dx = px - rx, dy = py - ry;
    const double a = dx * dx, b = dy * dy;
    return a + b;
}
// (d, i) replaces the running minimum: smaller, or equal with the lower index (a NaN never does)
FMPNP_SP_HD bool closer(double d, int i, double best, int best_i) { return d < best || (d == best && i < best_i); }
// the walk starts from (NO_DIST, NO_LANDMARK); when nothing replaced it (every distance NaN), landmark 0
constexpr double NO_DIST = __builtin_inf();
constexpr int NO_LANDMARK = INT32_MAX;
FMPNP_SP_HD int landmark_index(int best_i) { return best_i == NO_LANDMARK ? 0 : best_i; }

// match m of the list names reference keypoint j: its query row, or -1 when it is out of range
FMPNP_SP_HD bool match_valid(long long q, long long j, int N1, int N2) { return q >= 0 && q < N1 && j >= 0 && j < N2; }

// reference keypoint i, first matched by query row q, becomes row d of the assembled arrays
FMPNP_SP_HD void write_assembled(const double *query_pts, long long ld_q, const double *ref_pts, long long ld_r,
                                 const double *points3d, const int *argmin, int q, int i, int d, double *x2d,
                                 double *x2d_ref, double *x3d) {
    x2d[2 * (size_t)d] = query_pts[q];
    x2d[2 * (size_t)d + 1] = query_pts[ld_q + q];
    x2d_ref[2 * (size_t)d] = ref_pts[i];
    x2d_ref[2 * (size_t)d + 1] = ref_pts[ld_r + i];
    for (int k = 0; k < 3; ++k) x3d[3 * (size_t)d + k] = points3d[3 * (size_t)argmin[i] + k];
}

// ---- argument checks shared by the HIP entry points and the twins (host side) -----------------------------
inline int heat_args(const void *semi, int Hc, int Wc, const void *heat) {
    if (Hc < 0 || Wc < 0) return FMPNP_EINVAL;
    if (Hc * (long long)CELL > MAX_SIDE || Wc * (long long)CELL > MAX_SIDE) return FMPNP_ETOOBIG;
    if (Hc && Wc && (!semi || !heat)) return FMPNP_EINVAL;
    return 0;
}
inline int nms_args(const void *heat, int H, int W, double conf_thresh, int nms_dist, int border, const void *pts,
                    long long ld_pts) {
    if (H < 1 || W < 1 || nms_dist < 0 || border < 0 || !(conf_thresh == conf_thresh)) return FMPNP_EINVAL;
    if (H > MAX_SIDE || W > MAX_SIDE || nms_dist > MAX_DIST) return FMPNP_ETOOBIG;
    if (!heat || !pts || ld_pts < keep_capacity(H, W, nms_dist)) return FMPNP_EINVAL;
    return 0;
}
inline int desc_args(const void *coarse, int D, int Hc, int Wc, const void *pts, long long ld_pts, int N, int H, int W,
                     int align_corners, const void *desc, long long ld_desc) {
    if (D < 1 || Hc < 1 || Wc < 1 || N < 0 || H < 1 || W < 1 || ld_pts < N || ld_desc < N) return FMPNP_EINVAL;
    if (align_corners != 0 && align_corners != 1) return FMPNP_EINVAL;
    if (D > MAX_COUNT || N > MAX_COUNT || Hc > MAX_SIDE || Wc > MAX_SIDE) return FMPNP_ETOOBIG;
    if (N && (!coarse || !pts || !desc)) return FMPNP_EINVAL;
    return 0;
}
inline int match_args(const void *desc1, int N1, int ld1, const void *desc2_t, int D, int N2, int ld2, double ratio,
                      const void *nn_idx, const void *nn_dist, const void *ok, const void *matches, const void *count) {
    if (N1 < 0 || D < 1 || N2 < 2 || ld1 < D || ld2 < N2 || !(ratio == ratio)) return FMPNP_EINVAL;  // (topk(2) raises)
    if (N1 > MAX_COUNT || N2 > MAX_COUNT || D > MAX_COUNT) return FMPNP_ETOOBIG;
    if (!count) return FMPNP_EINVAL;
    if (N1 && (!desc1 || !desc2_t || !nn_idx || !nn_dist || !ok || !matches)) return FMPNP_EINVAL;
    return 0;
}
inline int assemble_args(const void *query_pts, int N1, long long ld_q, const void *ref_pts, int N2, long long ld_r,
                         const void *points2d, const void *points3d, int M, const void *matches, int n_matches,
                         const void *argmin, const void *x2d, const void *x2d_ref, const void *x3d, const void *count) {
    if (N1 < 0 || N2 < 0 || M < 0 || n_matches < 0 || ld_q < N1 || ld_r < N2) return FMPNP_EINVAL;
    if (N1 > MAX_COUNT || N2 > MAX_COUNT || M > MAX_COUNT || n_matches > MAX_COUNT) return FMPNP_ETOOBIG;
    if (!count) return FMPNP_EINVAL;
    if (N2 && M < 1) return FMPNP_EINVAL;  // (argmin over nothing raises)
    if (N2 && (!ref_pts || !points2d || !points3d || !argmin || !x2d || !x2d_ref || !x3d)) return FMPNP_EINVAL;
    if (n_matches && (!matches || !query_pts)) return FMPNP_EINVAL;
    return 0;
}

}  // namespace sp
}  // namespace fmpnp
