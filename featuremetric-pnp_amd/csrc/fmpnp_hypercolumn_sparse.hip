// fmpnp_hypercolumn_sparse.hip -- sparse hypercolumns: the descriptors of N points formed straight from the
// encoder's layers, without the dense [B][C][H][W] map (include/fmpnp.h, "Sparse hypercolumns", states the
// contract).  A texel of the assembly depends only on each layer's 2 x 2 taps at that texel, so every value
// here is the one fmpnp_hypercolumn.hip writes there: the same functions of fmpnp_hypercolumn_impl.h, the
// same 64-channel fp64 chains, no contraction.  The CPU twin (fmpnp_hypercolumn_sparse_cpu.cpp) calls them too.
//
// One workgroup of 4 waves per point (a grid-stride loop over the points, so N has no grid limit).  The point's
// texel, and with it every layer's taps and weights, is the same in every lane: scalar work, once per layer.
// The lanes run along the channels; every channel is another plane of the layer, so nothing coalesces and the
// game is loads in flight: each lane issues the four taps of HS_U of its channels before it uses any.
//   pass 1 (FMPNP_HC_NORMALIZE): the channels go through LDS in chunks of HS_CHUNK = 64 blocks of 64 -- the
//           lanes write their resized values, one lane per block walks its 64-long fp64 chain from LDS (the
//           rows are padded to 65 floats: the 64 walkers read 64 different banks), and every lane adds the
//           chunk's partials to its own copy of the running sum in ascending block order;
//   pass 2: every lane divides and stores, coalesced along out[p][.] -- from LDS when C fits one chunk,
//           otherwise recomputed with the same code chunk by chunk (the layers are then read twice, through
//           the caches).  The values are the same function of the same inputs either way: the path a launch
//           takes changes no bit.
// A bad point (include/fmpnp.h) writes a zero row and ORs the flag; no address is formed from it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fmpnp.h"
#include "fmpnp_hypercolumn_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {
namespace {

using namespace hc;

constexpr int HS_NT = 256;                      // 4 waves
constexpr int HS_CHUNK_BLOCKS = 64;             // one walker lane per block: one wave walks a chunk's chains
constexpr int HS_CHUNK = HS_CHUNK_BLOCKS * BLOCK;  // 4096 channels: 16.25 KB of LDS, several workgroups per CU
constexpr int HS_U = 4;                         // channels whose 4 taps a lane has in flight: 16 loads
constexpr unsigned HS_MAX_GRID = 1u << 16;

struct HsArgs {
    fmpnp_hc_layer layer[MAX_LAYERS];
    const void *points;
    const int *item;
    void *out;
    int *err;
    double p0, p1;
    size_t ld;
    int L, B, H, W, C, N, at, f64;
};

// body(c, v): the resized value v of concatenated channel c at texel (row, col) of item b, for this thread's
// share of [c_begin, c_end): each layer's segment of the range is dealt over the threads from its first channel
template <class F>
__device__ inline void walk(const HsArgs &a, int b, int row, int col, int c_begin, int c_end, int tid, F &&body) {
    int first = 0;  // the layer's first concatenated channel
    for (int l = 0; l < a.L && first < c_end; ++l) {
        const fmpnp_hc_layer &ly = a.layer[l];
        const int lo = max(c_begin, first), hi = min(c_end, first + ly.C);
        if (lo < hi) {
            const Tap ty = axis_tap(axis_scale(ly.H, a.H), ly.H, row), tx = axis_tap(axis_scale(ly.W, a.W), ly.W, col);
            const float *base = ly.data + (size_t)b * (size_t)ly.stride_b;
            const float *r0 = base + (size_t)ty.i0 * (size_t)ly.stride_y, *r1 = base + (size_t)ty.i1 * (size_t)ly.stride_y;
            const float *q00 = r0 + tx.i0, *q01 = r0 + tx.i1, *q10 = r1 + tx.i0, *q11 = r1 + tx.i1;
            const size_t cs = (size_t)ly.stride_c;
            int c = lo + tid;
            for (; c + (HS_U - 1) * HS_NT < hi; c += HS_U * HS_NT) {
                float t[HS_U][4];
#pragma unroll
                for (int u = 0; u < HS_U; ++u) {
                    const size_t off = (size_t)(c + u * HS_NT - first) * cs;
                    t[u][0] = q00[off];
                    t[u][1] = q01[off];
                    t[u][2] = q10[off];
                    t[u][3] = q11[off];
                }
#pragma unroll
                for (int u = 0; u < HS_U; ++u)
                    body(c + u * HS_NT, bilerp(t[u][0], t[u][1], t[u][2], t[u][3], tx.w0, tx.w1, ty.w0, ty.w1));
            }
            for (; c < hi; c += HS_NT) {
                const size_t off = (size_t)(c - first) * cs;
                body(c, bilerp(q00[off], q01[off], q10[off], q11[off], tx.w0, tx.w1, ty.w0, ty.w1));
            }
        }
        first += ly.C;
    }
}

__device__ inline void put(const HsArgs &a, size_t at, float v) {
    if (a.f64) ((double *)a.out)[at] = (double)v;
    else ((float *)a.out)[at] = v;
}

// a chunk-local channel's slot: rows of 64 padded to 65
__device__ inline int slot(int j) { return j + (j >> 6); }

template <bool NORM>
__global__ __launch_bounds__(HS_NT) void hypercolumn_sparse_kernel(const HsArgs a) {
    __shared__ float vals[HS_CHUNK + HS_CHUNK_BLOCKS];
    __shared__ double part[HS_CHUNK_BLOCKS];
    const int tid = (int)threadIdx.x;
    const bool one_chunk = a.C <= HS_CHUNK;
    for (int p = (int)blockIdx.x; p < a.N; p += (int)gridDim.x) {  // (p, and every branch on it, is the workgroup's)
        const size_t orow = (size_t)p * a.ld;
        int b, row, col;
        if (!locate(a.points, a.item, p, a.at, a.p0, a.p1, a.B, a.H, a.W, &b, &row, &col)) {
            for (int c = tid; c < a.C; c += HS_NT) put(a, orow + (size_t)c, 0.0f);
            if (tid == 0 && a.err) atomicOr(a.err, 1);
            continue;
        }
        if (!NORM) {
            walk(a, b, row, col, 0, a.C, tid, [&](int c, float v) { put(a, orow + (size_t)c, v); });
            continue;
        }
        double sum = 0.0;
        for (int c0 = 0; c0 < a.C; c0 += HS_CHUNK) {
            const int c1 = min(a.C, c0 + HS_CHUNK), nb = (c1 - c0 + BLOCK - 1) / BLOCK;
            walk(a, b, row, col, c0, c1, tid, [&](int c, float v) { vals[slot(c - c0)] = v; });
            __syncthreads();
            if (tid < nb) {
                const int n = min(BLOCK, c1 - c0 - tid * BLOCK);
                const float *v = vals + tid * (BLOCK + 1);
                double acc = 0.0;
                for (int i = 0; i < n; ++i) acc = square_acc(v[i], acc);
                part[tid] = acc;
            }
            __syncthreads();
            for (int j = 0; j < nb; ++j) sum = sum + part[j];
            // (the next chunk's values are written only after every lane has passed the second barrier, past
            // the walkers' reads; its partials only after the next first barrier, past these reads)
        }
        const float n = norm_of(sum);
        if (one_chunk) {
            for (int c = tid; c < a.C; c += HS_NT) put(a, orow + (size_t)c, normalised(vals[slot(c)], n));
            __syncthreads();  // (the next point overwrites vals)
        } else {
            walk(a, b, row, col, 0, a.C, tid, [&](int c, float v) { put(a, orow + (size_t)c, normalised(v, n)); });
        }
    }
}

}  // namespace

int launch_hypercolumn_sparse(const fmpnp_hc_layer *layers, int L, int B, int H, int W, const void *points,
                              const int *item, int N, int at, double p0, double p1, void *out, int dtype_out,
                              long long ld_out, long long C, int flags, int *err_flag, hipStream_t s) {
    if (N == 0) return 0;
    HsArgs a = {};
    for (int l = 0; l < L; ++l) a.layer[l] = layers[l];
    a.points = points;
    a.item = item;
    a.out = out;
    a.err = err_flag;
    a.p0 = p0;
    a.p1 = p1;
    a.ld = (size_t)ld_out;
    a.L = L;
    a.B = B;
    a.H = H;
    a.W = W;
    a.C = (int)C;
    a.N = N;
    a.at = at;
    a.f64 = dtype_out == FMPNP_F64;
    const dim3 grid(std::min<unsigned>((unsigned)N, HS_MAX_GRID)), block(HS_NT);
    if (flags & FMPNP_HC_NORMALIZE) hipLaunchKernelGGL(hypercolumn_sparse_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(hypercolumn_sparse_kernel<false>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace fmpnp
