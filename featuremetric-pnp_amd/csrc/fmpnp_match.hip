// fmpnp_match.hip -- dense exhaustive matching (s2dhm/pose_prediction/exhaustive_search.py:8-55) and
// the sparse-descriptor gather (s2dhm/pose_prediction/keypoint_association.py:40-86) on gfx950.
//
//   corr_kernel     scores[i][j] = sum_k sparse[i][k] * dense[k][j]: an LDS-tiled fp32 GEMM on
//                   v_mfma_f32_32x32x2_f32.  Every score is one accumulator's fmaf chain over
//                   k = 0 .. C-1 in ascending order from +0 (the MFMA is that chain bit for bit, and the
//                   zero-padded k tail adds fma(0, 0, acc)): no split-K, no atomics, so the value does
//                   not depend on the tile or the grid.
//   select_kernel   one workgroup per row: the flat argmax (lowest index among equal maxima, NaN above
//                   everything), d1 = the maximum and d_k = the top_k-th largest value by a radix
//                   select over an order-preserving 32-bit key, then the modified ratio test
//                   (float)(ratio^2) * d1 >= d_k (exhaustive_search.py:16-17).
//   gather_sparse_kernel   one wave per reference point: the descriptor of the nearest cell centre of
//                   generate_dense_keypoints' grid, in closed form per axis.
//
// The same key, select and mask run on the host in fmpnp_match_cpu.cpp (fmpnp_exhaustive_match_cpu).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "fmpnp.h"
#include "fmpnp_internal.h"

namespace fmpnp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- correlation ------------------------------------------------------------------------------
// 128 x 128 block of scores per workgroup, k in steps of 32; 4 waves, each 2 x 2 tiles of 32 x 32.
constexpr int BM = 128, BN = 128, BK = 32, CORR_NT = 256;
// LDS images, k-major: As[k][m] (the sparse tile transposed) and Bs[k][n].  A lane of the MFMA reads
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: 32 consecutive words of row k (lanes 0-31)
// and of row k + 1 (lanes 32-63).  As is written transposed (a wave's lanes run along k): the odd
// row stride spreads those writes over the banks.
constexpr int AS_LD = BM + 1, BS_LD = BN;
constexpr int A_PER_T = BM * BK / CORR_NT, B_PER_T = BK * BN / CORR_NT;  // 16 and 16

__global__ __launch_bounds__(CORR_NT) void corr_kernel(const float *__restrict__ sparse, int N, int ld_sparse,
                                                       const float *__restrict__ dense, int C, int WH,
                                                       int ld_dense, float *__restrict__ scores, size_t ld_scores,
                                                       int row_tiles, int xcd_order) {
    __shared__ float As[BK * AS_LD];
    __shared__ float Bs[BK * BS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Block -> tile: the hardware deals consecutive workgroup ids round-robin over the 8 XCDs, each with its
    // own L2.  Id = 8 * slot + xcd; an XCD's slots walk its own column tiles (xcd, xcd + 8, ...) with the
    // row tiles of one column tile adjacent, so a tile of the dense map (436 MB at the RobotCar shape, far
    // beyond any cache) comes from HBM once and serves every row tile from that XCD's L2.  (Which block
    // computes a tile changes no value.)
    // xcd_order = 0 (FMPNP_MATCH_XCD=0, measurement only): column tiles fastest, row tile by row tile.
    const int col_tiles8 = (WH + BN * 8 - 1) / (BN * 8) * 8;
    const int slot = blockIdx.x >> 3, xcd = blockIdx.x & 7;
    const int ct = xcd_order ? (slot / row_tiles) * 8 + xcd : (int)(blockIdx.x % col_tiles8);
    const int rt = xcd_order ? slot % row_tiles : (int)(blockIdx.x / col_tiles8);
    if (ct * BN >= WH) return;        // (the column tiles are padded to a multiple of 8)
    const int i0 = rt * BM;           // first row (sparse point) of the block
    const int j0 = ct * BN;           // first column (dense cell)
    // global -> register staging: A element e of this thread is (m = e * 8 + tid / 32, k = tid % 32),
    // B element e is (k = e * 2 + tid / 128, n = tid % 128); out-of-range elements are zero.  (Unconditional
    // dword loads: 16-byte loads behind an alignment-and-range branch measured a third slower)
    const int a_k = tid & 31, a_m = tid >> 5;
    const int b_n = tid & 127, b_k = tid >> 7;
    float ra[A_PER_T], rb[B_PER_T];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < A_PER_T; ++e) {
            const int m = i0 + e * 8 + a_m, k = k0 + a_k;
            ra[e] = (m < N && k < C) ? sparse[(size_t)m * ld_sparse + k] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < B_PER_T; ++e) {
            const int k = k0 + e * 2 + b_k, n = j0 + b_n;
            rb[e] = (k < C && n < WH) ? dense[(size_t)k * ld_dense + n] : 0.f;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    fetch(0);
    for (int k0 = 0; k0 < C; k0 += BK) {
        __syncthreads();  // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < A_PER_T; ++e) As[a_k * AS_LD + e * 8 + a_m] = ra[e];
#pragma unroll
        for (int e = 0; e < B_PER_T; ++e) Bs[(e * 2 + b_k) * BS_LD + b_n] = rb[e];
        __syncthreads();
        if (k0 + BK < C) fetch(k0 + BK);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = As[(kk + h) * AS_LD + wm + r], a1 = As[(kk + h) * AS_LD + wm + 32 + r];
            const float b0 = Bs[(kk + h) * BS_LD + wn + r], b1 = Bs[(kk + h) * BS_LD + wn + 32 + r];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = j0 + wn + b * 32 + r;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = i0 + wm + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
                if (row < N && col < WH) scores[(size_t)row * ld_scores + col] = acc[a][b][g];
            }
        }
}

// ---- row reduction ----------------------------------------------------------------------------
constexpr int SEL_NT = 1024;  // 16 waves per row: the passes are bound by load latency

// Order-preserving key (also in fmpnp_match_cpu.cpp): every NaN is the greatest key, -0 counts as +0.
__device__ inline unsigned score_key(float x) {
    if (x != x) return 0xffffffffu;
    const unsigned u = __float_as_uint(x + 0.f);  // (-0 + +0 = +0)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key_score(unsigned key) {
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__global__ __launch_bounds__(SEL_NT) void select_kernel(const float *__restrict__ scores, size_t ld_scores, int WH,
                                                        int top_k, float ratio2, int *__restrict__ argmax,
                                                        float *__restrict__ top, float *__restrict__ kth,
                                                        unsigned char *__restrict__ mask) {
    __shared__ unsigned hist[256], scan[256];
    __shared__ unsigned long long wbest[SEL_NT / 64];
    __shared__ unsigned s_prefix, s_want;
    const int tid = threadIdx.x;
    const float *row = scores + (size_t)blockIdx.x * ld_scores;
    const bool vec = (WH & 3) == 0 && ((uintptr_t)row & 15) == 0;  // 16-byte loads where the row allows
    unsigned prefix = 0, want = (unsigned)top_k;  // the want-th largest among the keys matching prefix
    unsigned long long best = 0;                   // (key << 32) | ~index: max = greatest key, lowest index
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        auto take = [&](float x, int j) {
            const unsigned key = score_key(x);
            if (pass == 0) {
                const unsigned long long v = ((unsigned long long)key << 32) | (unsigned)~(unsigned)j;
                best = v > best ? v : best;
                atomicAdd(&hist[key >> 24], 1u);
            } else if ((key >> (shift + 8)) == (prefix >> (shift + 8))) {
                atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
        };
        if (vec) {
            for (int j = tid * 4; j < WH; j += SEL_NT * 4) {
                const float4 v = *(const float4 *)(row + j);
                take(v.x, j);
                take(v.y, j + 1);
                take(v.z, j + 2);
                take(v.w, j + 3);
            }
        } else {
            for (int j = tid; j < WH; j += SEL_NT) take(row[j], j);
        }
        __syncthreads();
        // the bin in which the want-th largest key falls: scan[b] = the count of bins b .. 255 (a suffix
        // scan in LDS by the first 256 threads), and the bin is the one with scan[b + 1] < want <= scan[b]
        if (tid < 256) scan[tid] = hist[tid];
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned v = (tid < 256 && tid + off < 256) ? scan[tid + off] : 0u;
            __syncthreads();
            if (tid < 256) scan[tid] += v;
            __syncthreads();
        }
        if (tid < 256) {
            const unsigned incl = scan[tid], excl = incl - hist[tid];
            if (excl < want && want <= incl) {  // (exactly one bin: an empty bin has excl == incl)
                s_prefix = prefix | ((unsigned)tid << shift);
                s_want = want - excl;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        want = s_want;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(best, o, 64);
        best = v > best ? v : best;
    }
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SEL_NT / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
        const float d1 = key_score((unsigned)(best >> 32)), dk = key_score(prefix);
        argmax[blockIdx.x] = (int)~(unsigned)best;
        top[blockIdx.x] = d1;
        kth[blockIdx.x] = dk;
        mask[blockIdx.x] = __fmul_rn(ratio2, d1) >= dk ? 1 : 0;
    }
}

// ---- sparse-descriptor gather -----------------------------------------------------------------
// The grid of generate_dense_keypoints (keypoint_association.py:26-38): centre i * cell + cell / 2
// per axis; point coordinate 0 runs along the map's last dimension, coordinate 1 along the first.
// fast_closest_points' argmin (:77-86) takes the lower cell on an exact edge (the first minimum).
__device__ inline int nearest_cell(double p, double cell, int n) {
    const double c = ceil(p / cell - 1.0);
    return c > 0.0 ? (c < (double)(n - 1) ? (int)c : n - 1) : 0;  // (NaN: cell 0)
}

__global__ __launch_bounds__(256) void gather_sparse_kernel(const float *__restrict__ chw, int C, int D1, int D2,
                                                            const double *__restrict__ pts, int N, double cell0,
                                                            double cell1, float *__restrict__ out, int ld_out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= N) return;
    const int ia = nearest_cell(pts[2 * (size_t)p], cell1, D2);      // coordinate 0: the last dimension
    const int ib = nearest_cell(pts[2 * (size_t)p + 1], cell0, D1);  // coordinate 1: the first dimension
    const size_t plane = (size_t)D1 * D2, cell = (size_t)ib * D2 + ia;
    for (int c = lane; c < C; c += 64) out[(size_t)p * ld_out + c] = chw[c * plane + cell];
}

}  // namespace

hipError_t launch_corr(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                       float *scores, size_t ld_scores, hipStream_t s) {
    const int row_tiles = (N + BM - 1) / BM, col_tiles = (WH + BN - 1) / BN;
    const size_t blocks = (size_t)((col_tiles + 7) / 8) * 8 * (size_t)row_tiles;
    if (blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    const char *env = getenv("FMPNP_MATCH_XCD");  // measurement knob, read per launch
    const int xcd_order = !(env && env[0] == '0');
    hipLaunchKernelGGL(corr_kernel, dim3((unsigned)blocks), dim3(CORR_NT), 0, s, sparse, N, ld_sparse, dense, C, WH,
                       ld_dense, scores, ld_scores, row_tiles, xcd_order);
    return hipGetLastError();
}

hipError_t launch_select(const float *scores, size_t ld_scores, int N, int WH, int top_k, float ratio2, int *argmax,
                         float *top, float *kth, unsigned char *mask, hipStream_t s) {
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)N), dim3(SEL_NT), 0, s, scores, ld_scores, WH, top_k, ratio2,
                       argmax, top, kth, mask);
    return hipGetLastError();
}

hipError_t launch_gather_sparse(const float *chw, int C, int D1, int D2, const double *pts, int N, double cell0,
                                double cell1, float *out, int ld_out, hipStream_t s) {
    hipLaunchKernelGGL(gather_sparse_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, chw, C, D1, D2, pts, N,
                       cell0, cell1, out, ld_out);
    return hipGetLastError();
}

int dense_match_args(const void *sparse, int N, int ld_sparse, const void *dense, int C, int WH, int ld_dense, int top_k,
                     double ratio, const void *argmax, const void *top, const void *kth, const void *mask) {
    if (N < 0 || C <= 0 || WH <= 0 || ld_sparse < C || ld_dense < WH) return FMPNP_EINVAL;
    if (top_k < 1 || top_k > WH || !(ratio == ratio)) return FMPNP_EINVAL;  // (the reference: IndexError)
    if (WH > INT32_MAX - (1 << 16)) return FMPNP_ETOOBIG;  // (32-bit column indices with the loops' strides)
    if (N > 0 && (!sparse || !dense || !argmax || !top || !kth || !mask)) return FMPNP_EINVAL;
    return 0;
}

}  // namespace fmpnp

using namespace fmpnp;

namespace {

// Rows per correlation + select round: the score workspace holds this many rows (256 MB at most, one
// row at least), so it stays bounded however many rows a call brings.
constexpr size_t MATCH_WS_CAP = (size_t)256 << 20;
inline int match_chunk_rows(int N, int WH) {
    const size_t rows = std::max<size_t>(1, MATCH_WS_CAP / ((size_t)WH * sizeof(float)));
    return (int)std::min<size_t>(rows, (size_t)std::max(N, 1));
}

}  // namespace

extern "C" {

size_t fmpnp_match_workspace_size(int N, int WH) {
    if (N <= 0 || WH <= 0) return 0;
    return (size_t)match_chunk_rows(N, WH) * (size_t)WH * sizeof(float);
}

int fmpnp_exhaustive_match_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                 int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                 unsigned char *mask, float *scores, void *workspace, size_t workspace_bytes,
                                 void *hip_stream) {
    const int rc = dense_match_args(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!scores && (!workspace || workspace_bytes < fmpnp_match_workspace_size(N, WH))) return FMPNP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    const float ratio2 = (float)(ratio * ratio);  // exhaustive_search.py:17: a Python float times an fp32 tensor
    const int chunk = match_chunk_rows(N, WH);
    for (int i0 = 0; i0 < N; i0 += chunk) {  // (stream order: a round's select reads before the next round writes)
        const int n = std::min(chunk, N - i0);
        float *dst = scores ? scores + (size_t)i0 * WH : (float *)workspace;
        hipError_t e = launch_corr(sparse + (size_t)i0 * ld_sparse, n, ld_sparse, dense, C, WH, ld_dense, dst,
                                   (size_t)WH, s);
        if (e != hipSuccess) return (int)e;
        e = launch_select(dst, (size_t)WH, n, WH, top_k, ratio2, argmax + i0, top + i0, kth + i0, mask + i0, s);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

int fmpnp_correlation_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                            float *scores, void *hip_stream) {
    if (N < 0 || C <= 0 || WH <= 0 || ld_sparse < C || ld_dense < WH) return FMPNP_EINVAL;
    if (WH > INT32_MAX - (1 << 16)) return FMPNP_ETOOBIG;
    if (N == 0) return 0;
    if (!sparse || !dense || !scores) return FMPNP_EINVAL;
    return (int)launch_corr(sparse, N, ld_sparse, dense, C, WH, ld_dense, scores, (size_t)WH, (hipStream_t)hip_stream);
}

int fmpnp_exhaustive_match(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                           int top_k, double ratio, int *argmax, float *top, float *kth, unsigned char *mask,
                           float *scores_dev, void *hip_stream) {
    return fmpnp_exhaustive_match_ex(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask,
                                     scores_dev, FMPNP_MATCH_F32, hip_stream);
}

int fmpnp_gather_sparse_descriptors(const float *dense_chw, int C, int D1, int D2, const double *points2d, int N,
                                    double cell0, double cell1, float *out, int ld_out, void *hip_stream) {
    if (N < 0 || C <= 0 || D1 <= 0 || D2 <= 0 || ld_out < C) return FMPNP_EINVAL;
    if (!(cell0 > 0.0) || !(cell1 > 0.0) || isinf(cell0) || isinf(cell1)) return FMPNP_EINVAL;
    if ((size_t)D1 * (size_t)D2 > (size_t)INT32_MAX) return FMPNP_ETOOBIG;
    if (N == 0) return 0;
    if (!dense_chw || !points2d || !out) return FMPNP_EINVAL;
    return (int)launch_gather_sparse(dense_chw, C, D1, D2, points2d, N, cell0, cell1, out, ld_out,
                                     (hipStream_t)hip_stream);
}

}  // extern "C"
