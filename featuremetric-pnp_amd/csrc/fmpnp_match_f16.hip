// fmpnp_match_f16.hip -- the opt-in fp16 precision of the dense matching stage (FMPNP_MATCH_F16,
// include/fmpnp.h "fp16 precision") on gfx950, and the precision-taking entry points of the stage.
//
//   cvt_sparse_kernel   sparse [N][ld] fp32 -> fp16 rows [N][Cp] (row-major, Cp = C rounded up to the
//                       k-tile, the tail zero): one thread per 8 consecutive k, one 16-byte store.
//   cvt_dense_kernel    dense [C][ld] fp32 -> fp16 k-blocked [Cp / 8][WH][8]: element j of the 16-byte
//                       unit (kb, col) is dense[8 kb + j][col], zero for 8 kb + j >= C.  A lane's B fragment
//                       of v_mfma_f32_32x32x16_f16 (B[k = 8 (l >> 5) + j][col l & 31]) is one such unit.
//                       Both read dword by dword (no alignment is assumed of the fp32 operands) and round
//                       with v_cvt_f16_f32 (nearest-even, NaN / Inf kept, beyond 65504 -> Inf).
//   corr_f16_kernel     scores[i][j] = sum_k fl16(sparse[i][k]) * fl16(dense[k][j]), fp32 accumulation by
//                       v_mfma_f32_32x32x16_f16: an LDS-tiled GEMM, 128 x 128 scores per workgroup, k in
//                       tiles of 64 taken in ascending order into one accumulator per score (no split-K, no
//                       atomics), two LDS buffers and one barrier per k-tile.  Which block, tile or round
//                       computes a score changes no bit of it: a score sees the same sequence of 16-deep
//                       MFMA steps over k = 0 .. Cp - 1 wherever it lands.
//
// The row reduction is fmpnp_match.hip's select_kernel on these scores, unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fmpnp.h"
#include "fmpnp_internal.h"

namespace fmpnp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // a 16-byte unit: 8 fp16 values

constexpr int HM = 128, HN = 128, HK = 64, H_NT = 256;  // block of scores, k-tile, threads (4 waves of 64 x 64)
constexpr int KB = HK / 8;                               // 16-byte k-blocks per k-tile
constexpr int A_PER_T = HM * KB / H_NT, B_PER_T = HN * KB / H_NT;  // 4 and 4 units per thread per k-tile
constexpr int CVT_NT = 256;

__host__ __device__ inline int padded_c(int C) { return (int)(((long long)C + HK - 1) / HK * HK); }

__global__ __launch_bounds__(CVT_NT) void cvt_sparse_kernel(const float *__restrict__ src, int N, int C, int ld,
                                                            u32x4 *__restrict__ dst, int units) {
    const int u = blockIdx.x * CVT_NT + threadIdx.x;  // the unit (8 k) of the row
    if (u >= units) return;
    for (int i = blockIdx.y; i < N; i += gridDim.y) {
        const float *row = src + (size_t)i * ld;
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = u * 8 + j;
            v[j] = (_Float16)(k < C ? row[k] : 0.f);
        }
        dst[(size_t)i * units + u] = __builtin_bit_cast(u32x4, v);
    }
}

__global__ __launch_bounds__(CVT_NT) void cvt_dense_kernel(const float *__restrict__ src, int C, int WH, int ld,
                                                           u32x4 *__restrict__ dst, int kblocks) {
    const int col = blockIdx.x * CVT_NT + threadIdx.x;
    if (col >= WH) return;
    for (int kb = blockIdx.y; kb < kblocks; kb += gridDim.y) {
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = kb * 8 + j;
            v[j] = (_Float16)(k < C ? src[(size_t)k * ld + col] : 0.f);
        }
        dst[(size_t)kb * WH + col] = __builtin_bit_cast(u32x4, v);
    }
}

// LDS images of one k-tile, in 16-byte units: As[kb][m] and Bs[kb][n].  A lane of the MFMA step s reads the
// units (kb = 2 s + (l >> 5), row or column l & 31): 32 consecutive units, conflict-free.  The B units are
// written as they are read (a wave's lanes run along n).  The A units are written with a wave's lanes running
// along kb (8 lanes cover a row's 128 bytes in global memory), so m is XOR-ed with 2 kb: the 16 lanes of a
// write group then fall on 16 different 16-byte bank slots, and a read group is permuted within itself.
__device__ inline int a_unit(int kb, int m) { return kb * HM + (m ^ (2 * kb)); }

__global__ __launch_bounds__(H_NT) void corr_f16_kernel(const u32x4 *__restrict__ sparse16, int N, int units_a,
                                                        const u32x4 *__restrict__ dense16, int WH, int k_tiles,
                                                        float *__restrict__ scores, size_t ld_scores, int row_tiles) {
    __shared__ u32x4 As[2][KB * HM];
    __shared__ u32x4 Bs[2][KB * HN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block -> tile as fmpnp_match.hip's corr_kernel: id = 8 * slot + xcd, an XCD's slots walk its own column
    // tiles with the row tiles of one column tile adjacent, so a tile of the dense image comes from HBM once
    const int slot = blockIdx.x >> 3, xcd = blockIdx.x & 7;
    const int ct = (slot / row_tiles) * 8 + xcd, rt = slot % row_tiles;
    if (ct * HN >= WH) return;  // (the column tiles are padded to a multiple of 8; the whole block leaves)
    const int i0 = rt * HM, j0 = ct * HN;
    // global -> register staging, 16 bytes per load: A unit e of this thread is (m = e * 32 + tid / 8,
    // kb = tid % 8), B unit e is (kb = e * 2 + tid / 128, n = tid % 128); rows >= N and columns >= WH are zero
    const int a_kb = tid & 7, a_m = tid >> 3;
    const int b_n = tid & 127, b_kb = tid >> 7;
    u32x4 ra[A_PER_T], rb[B_PER_T];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    auto fetch = [&](int t) {
#pragma unroll
        for (int e = 0; e < A_PER_T; ++e) {
            const int m = i0 + e * 32 + a_m;
            ra[e] = m < N ? sparse16[(size_t)m * units_a + (size_t)t * KB + a_kb] : zero;
        }
#pragma unroll
        for (int e = 0; e < B_PER_T; ++e) {
            const int n = j0 + b_n;
            rb[e] = n < WH ? dense16[((size_t)t * KB + e * 2 + b_kb) * (size_t)WH + n] : zero;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int e = 0; e < A_PER_T; ++e) As[buf][a_unit(a_kb, e * 32 + a_m)] = ra[e];
#pragma unroll
        for (int e = 0; e < B_PER_T; ++e) Bs[buf][(e * 2 + b_kb) * HN + b_n] = rb[e];
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int t = 0; t < k_tiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < k_tiles) fetch(t + 1);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int s = 0; s < HK / 16; ++s) {
            const int kb = 2 * s + h;
            const f16x8 a0 = __builtin_bit_cast(f16x8, As[buf][a_unit(kb, wm + r)]);
            const f16x8 a1 = __builtin_bit_cast(f16x8, As[buf][a_unit(kb, wm + 32 + r)]);
            const f16x8 b0 = __builtin_bit_cast(f16x8, Bs[buf][kb * HN + wn + r]);
            const f16x8 b1 = __builtin_bit_cast(f16x8, Bs[buf][kb * HN + wn + 32 + r]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
        }
        // the other buffer was last read in the previous iteration, before its closing barrier
        if (t + 1 < k_tiles) stage(buf ^ 1);
        __syncthreads();
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

inline size_t sparse16_bytes(int N, int C) { return align256((size_t)N * (size_t)padded_c(C) * 2); }
inline size_t dense16_bytes(int C, int WH) { return align256((size_t)padded_c(C) * (size_t)WH * 2); }

hipError_t launch_cvt_sparse(const float *sparse, int N, int C, int ld, void *dst, hipStream_t s) {
    const int units = padded_c(C) / 8;
    hipLaunchKernelGGL(cvt_sparse_kernel, dim3((unsigned)((units + CVT_NT - 1) / CVT_NT), (unsigned)std::min(N, 65535)),
                       dim3(CVT_NT), 0, s, sparse, N, C, ld, (u32x4 *)dst, units);
    return hipGetLastError();
}

hipError_t launch_cvt_dense(const float *dense, int C, int WH, int ld, void *dst, hipStream_t s) {
    const int kblocks = padded_c(C) / 8;
    hipLaunchKernelGGL(cvt_dense_kernel, dim3((unsigned)((WH + CVT_NT - 1) / CVT_NT), (unsigned)std::min(kblocks, 65535)),
                       dim3(CVT_NT), 0, s, dense, C, WH, ld, (u32x4 *)dst, kblocks);
    return hipGetLastError();
}

// rows [0, N) of the fp16 sparse image x the fp16 dense image -> scores [N][ld_scores]
hipError_t launch_corr_f16(const void *sparse16, int N, int C, const void *dense16, int WH, float *scores,
                           size_t ld_scores, hipStream_t s) {
    const int row_tiles = (N + HM - 1) / HM, col_tiles = (WH + HN - 1) / HN;
    const size_t blocks = (size_t)((col_tiles + 7) / 8) * 8 * (size_t)row_tiles;
    if (blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(corr_f16_kernel, dim3((unsigned)blocks), dim3(H_NT), 0, s, (const u32x4 *)sparse16, N,
                       padded_c(C) / 8, (const u32x4 *)dense16, WH, padded_c(C) / HK, scores, ld_scores, row_tiles);
    return hipGetLastError();
}

// (fmpnp_match.hip's round: as many rows as its workspace holds)
inline int chunk_rows(int N, int WH) { return (int)(fmpnp_match_workspace_size(N, WH) / ((size_t)WH * sizeof(float))); }

int shape_args(int N, int C, int WH, int ld_sparse, int ld_dense) {
    if (N < 0 || C <= 0 || WH <= 0 || ld_sparse < C || ld_dense < WH) return FMPNP_EINVAL;
    if (WH > INT32_MAX - (1 << 16) || C > INT32_MAX - HK) return FMPNP_ETOOBIG;
    return 0;
}

// the fp16 precision's argument checks (its own order: the size bounds before top_k)
int match_args_f16(const void *sparse, int N, int ld_sparse, const void *dense, int C, int WH, int ld_dense, int top_k,
                   double ratio, const void *argmax, const void *top, const void *kth, const void *mask) {
    const int rc = shape_args(N, C, WH, ld_sparse, ld_dense);
    if (rc) return rc;
    if (top_k < 1 || top_k > WH || !(ratio == ratio)) return FMPNP_EINVAL;
    if (N > 0 && (!sparse || !dense || !argmax || !top || !kth || !mask)) return FMPNP_EINVAL;
    return 0;
}

// both operands -> their fp16 images at the head of the workspace ([dense][sparse]); the bytes they take
int convert_operands(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                     unsigned char *ws, hipStream_t s) {
    hipError_t e = launch_cvt_dense(dense, C, WH, ld_dense, ws, s);
    if (e == hipSuccess) e = launch_cvt_sparse(sparse, N, C, ld_sparse, ws + dense16_bytes(C, WH), s);
    return (int)e;
}

}  // namespace

}  // namespace fmpnp

using namespace fmpnp;

extern "C" {

size_t fmpnp_match_workspace_size_ex(int N, int C, int WH, int precision) {
    if (precision == FMPNP_MATCH_F32) return fmpnp_match_workspace_size(N, WH);
    if (precision != FMPNP_MATCH_F16 || N <= 0 || C <= 0 || WH <= 0 || C > INT32_MAX - HK) return 0;
    return dense16_bytes(C, WH) + sparse16_bytes(N, C) + align256(fmpnp_match_workspace_size(N, WH));
}

int fmpnp_exhaustive_match_ex_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                    int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                    unsigned char *mask, float *scores, void *workspace, size_t workspace_bytes,
                                    int precision, void *hip_stream) {
    if (precision == FMPNP_MATCH_F32)
        return fmpnp_exhaustive_match_async(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth,
                                            mask, scores, workspace, workspace_bytes, hip_stream);
    if (precision != FMPNP_MATCH_F16) return FMPNP_EINVAL;
    const int rc = match_args_f16(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask);
    if (rc) return rc;
    if (N == 0) return 0;
    const size_t b_img = dense16_bytes(C, WH) + sparse16_bytes(N, C);
    const size_t need = scores ? b_img : fmpnp_match_workspace_size_ex(N, C, WH, precision);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) return FMPNP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    unsigned char *ws = (unsigned char *)workspace;
    int e = convert_operands(sparse, N, ld_sparse, dense, C, WH, ld_dense, ws, s);  // once per call
    if (e) return e;
    const unsigned char *dense16 = ws, *sparse16 = ws + dense16_bytes(C, WH);
    const float ratio2 = (float)(ratio * ratio);
    const int chunk = chunk_rows(N, WH);
    const size_t row16 = (size_t)padded_c(C) * 2;
    for (int i0 = 0; i0 < N; i0 += chunk) {  // (stream order: a round's select reads before the next round writes)
        const int n = std::min(chunk, N - i0);
        float *dst = scores ? scores + (size_t)i0 * WH : (float *)(ws + b_img);
        hipError_t he = launch_corr_f16(sparse16 + (size_t)i0 * row16, n, C, dense16, WH, dst, (size_t)WH, s);
        if (he != hipSuccess) return (int)he;
        he = launch_select(dst, (size_t)WH, n, WH, top_k, ratio2, argmax + i0, top + i0, kth + i0, mask + i0, s);
        if (he != hipSuccess) return (int)he;
    }
    return 0;
}

int fmpnp_correlation_ex_async(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                               float *scores, void *workspace, size_t workspace_bytes, int precision, void *hip_stream) {
    if (precision == FMPNP_MATCH_F32)
        return fmpnp_correlation_async(sparse, N, ld_sparse, dense, C, WH, ld_dense, scores, hip_stream);
    if (precision != FMPNP_MATCH_F16) return FMPNP_EINVAL;
    const int rc = shape_args(N, C, WH, ld_sparse, ld_dense);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!sparse || !dense || !scores) return FMPNP_EINVAL;
    const size_t b_img = dense16_bytes(C, WH) + sparse16_bytes(N, C);
    if (!workspace || workspace_bytes < b_img || ((uintptr_t)workspace & 15)) return FMPNP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    unsigned char *ws = (unsigned char *)workspace;
    const int e = convert_operands(sparse, N, ld_sparse, dense, C, WH, ld_dense, ws, s);
    if (e) return e;
    return (int)launch_corr_f16(ws + dense16_bytes(C, WH), N, C, ws, WH, scores, (size_t)WH, s);
}

// the synchronous call of both precisions (fmpnp_exhaustive_match forwards here with FMPNP_MATCH_F32): each
// precision's own argument checks and workspace, then one carve, one run and one download
int fmpnp_exhaustive_match_ex(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                              int top_k, double ratio, int *argmax, float *top, float *kth, unsigned char *mask,
                              float *scores_dev, int precision, void *hip_stream) {
    const bool f16 = precision == FMPNP_MATCH_F16;
    if (!f16 && precision != FMPNP_MATCH_F32) return FMPNP_EINVAL;
    const int rc0 = f16 ? match_args_f16(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask)
                        : dense_match_args(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask);
    if (rc0) return rc0;
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    // the caller's scores_dev takes the score rows' place: then only the fp16 images remain, or nothing
    const size_t b_ws = f16 ? (scores_dev ? dense16_bytes(C, WH) + sparse16_bytes(N, C)
                                          : fmpnp_match_workspace_size_ex(N, C, WH, precision))
                            : (scores_dev ? 0 : align256(fmpnp_match_workspace_size(N, WH)));
    const size_t b_i = align256(sizeof(int) * (size_t)N), b_f = align256(sizeof(float) * (size_t)N), b_m = align256((size_t)N);
    SyncCall call(SCRATCH_MATCH, s, b_ws + b_i + 2 * b_f + b_m, 0);
    if (call.error()) return call.error();
    unsigned char *base = call.dev;
    int *d_arg = (int *)(base + b_ws);
    float *d_top = (float *)(base + b_ws + b_i), *d_kth = (float *)(base + b_ws + b_i + b_f);
    unsigned char *d_mask = base + b_ws + b_i + 2 * b_f;
    const int rc = fmpnp_exhaustive_match_ex_async(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, d_arg, d_top,
                                                   d_kth, d_mask, scores_dev, base, b_ws, precision, hip_stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(argmax, d_arg, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(top, d_top, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(kth, d_kth, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(mask, d_mask, (size_t)N, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    return call.finish();
}

}  // extern "C"
