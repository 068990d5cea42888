// fmpnp_pnp.hip -- P3P RANSAC + reprojection polish on gfx950 (include/fmpnp.h, "initial pose";
// s2dhm/pose_prediction/solve_pnp.py:44-69).  Two kernels per call, B problems each:
//
//   pnp_hyp_kernel       grid (ceil(max iters / 256), B): one lane owns one hypothesis -- it samples,
//                        solves P3P, lets the fourth point pick the solution, then tests the problem's M
//                        points, staged through LDS 256 at a time (every lane reads the same point: a
//                        broadcast), and counts.
//                        The workgroup's keys (count << 32 | ~h) are reduced by an integer maximum in
//                        LDS and one 64-bit atomic maximum per workgroup lands in the problem's key.
//   pnp_finalise_kernel  one 256-lane workgroup per problem: re-derives the best hypothesis from
//                        (seed, h) -- no poses are stored -- writes the mask and runs the polish, whose
//                        28 sums are reduced in the fixed order of the header.
//
// Every value is computed by fmpnp_pnp_impl.h, which the CPU twin shares.
#include <string.h>

#include <algorithm>
#include <vector>

#include "fmpnp_internal.h"
#include "fmpnp_pnp_impl.h"

namespace fmpnp {
namespace {

using namespace pnp;

constexpr int PNP_NT = POLISH_LANES;  // 256 lanes: the hypothesis kernel's and the polish's workgroup

constexpr int TILE = PNP_NT;  // points staged in LDS per round: one per lane, 48 B each
struct alignas(16) TilePoint {
    double X[3], pad, x[2];
};

// the inliers of (R, t) among the n staged points (every lane reads the same point: LDS broadcasts)
template <bool ND>
__device__ __forceinline__ int count_tile(const Cam &cam, const double *R, const double *t, const TilePoint *tile,
                                          int n, double thr2) {
    int count = 0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) count += is_inlier_t<ND>(cam, R, t, tile[j].X, tile[j].x, thr2) ? 1 : 0;
    return count;
}

__global__ __launch_bounds__(PNP_NT) void pnp_hyp_kernel(const fmpnp_pnp_problem *__restrict__ probs,
                                                         unsigned long long *__restrict__ keys) {
    __shared__ TilePoint tile[TILE];
    __shared__ unsigned long long skey[PNP_NT];
    const fmpnp_pnp_problem &p = probs[blockIdx.y];
    const int M = p.M, iters = p.iters;
    if (M < 4 || (long long)blockIdx.x * PNP_NT >= (long long)iters) return;  // (uniform: before any barrier)
    const int tid = threadIdx.x;
    const unsigned h = blockIdx.x * PNP_NT + tid;
    const Cam cam = make_cam(p.K, p.dist);
    const double *__restrict__ p3 = p.points3d, *__restrict__ p2 = p.points2d;
    const double thr2 = p.threshold * p.threshold;
    double R[9], t[3];
    const bool have = h < (unsigned)iters && hypothesis(cam, p3, p2, M, p.seed, h, R, t);
    int count = 0;
    // the M points pass through LDS in rounds of TILE (any M: there is no staging cap); a point read
    // straight from global memory costs every lane a full memory latency per test
    for (int base = 0; base < M; base += TILE) {
        if (base) __syncthreads();  // (the previous round's readers are done)
        const int i = base + tid;
        if (i < M) {
            for (int k = 0; k < 3; ++k) tile[tid].X[k] = p3[3 * (size_t)i + k];
            for (int k = 0; k < 2; ++k) tile[tid].x[k] = p2[2 * (size_t)i + k];
        }
        __syncthreads();
        const int n = min(TILE, M - base);
        if (have) count += cam.nodist ? count_tile<true>(cam, R, t, tile, n, thr2) : count_tile<false>(cam, R, t, tile, n, thr2);
    }
    skey[tid] = h < (unsigned)iters ? pack_key(count, h) : 0ull;
    __syncthreads();
    for (int s = PNP_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const unsigned long long o = skey[tid + s];
            if (o > skey[tid]) skey[tid] = o;
        }
        __syncthreads();
    }
    if (tid == 0) atomicMax(&keys[blockIdx.y], skey[0]);
}

// the polish's sums over the workgroup: lane l accumulates its points, then the tree of the header
struct BlockEval {
    const Cam &cam;
    const double *p3, *p2;
    const unsigned char *mask;
    int M, tid;
    double *sh;  // [NACC][PNP_NT]
    __device__ void operator()(const double *R, const double *t, double *S) {
        double acc[NACC];
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
        for (int i = tid; i < M; i += PNP_NT)
            if (mask[i]) polish_point(cam, R, t, p3 + 3 * (size_t)i, p2 + 2 * (size_t)i, acc);
        for (int k = 0; k < NACC; ++k) sh[k * PNP_NT + tid] = acc[k];
        __syncthreads();
        // lane l += lane l + s for s = 128 .. 1, each of the NACC sums: the s * NACC additions of a level are
        // dealt over all the lanes (the same pairs are added, so the same bits)
        for (int s = PNP_NT / 2; s > 0; s >>= 1) {
            for (int idx = tid; idx < s * NACC; idx += PNP_NT) {
                const int k = idx / s, l = idx - k * s;
                sh[k * PNP_NT + l] = sh[k * PNP_NT + l] + sh[k * PNP_NT + l + s];
            }
            __syncthreads();
        }
        for (int k = 0; k < NACC; ++k) S[k] = sh[k * PNP_NT];
        __syncthreads();  // (the next evaluation overwrites sh)
    }
};

__global__ __launch_bounds__(PNP_NT) void pnp_finalise_kernel(const fmpnp_pnp_problem *__restrict__ probs,
                                                              const unsigned long long *__restrict__ keys,
                                                              fmpnp_pnp_result *__restrict__ results,
                                                              unsigned char *__restrict__ mask_all) {
    __shared__ double sh[NACC * PNP_NT];
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x;
    const fmpnp_pnp_problem &p = probs[b];
    fmpnp_pnp_result &res = results[b];
    const int M = p.M;
    if (M < 4) {
        if (tid == 0) res.status = FMPNP_PNP_TOO_FEW;
        return;
    }
    unsigned char *mask = mask_all + p.mask_offset;
    const unsigned long long key = keys[b];
    const int best_count = (int)(key >> 32);
    if (best_count == 0) {
        for (int i = tid; i < M; i += PNP_NT) mask[i] = 0;
        if (tid == 0) {
            for (int k = 0; k < 9; ++k) res.R[k] = res.R_hyp[k] = 0.0;
            for (int k = 0; k < 3; ++k) res.t[k] = res.t_hyp[k] = 0.0;
            res.cost = 0.0;
            res.num_inliers = 0;
            res.best_h = -1;
            res.status = FMPNP_PNP_NO_MODEL;
            res.polish_iters = 0;
        }
        return;
    }
    const unsigned h = ~(unsigned)key;
    const Cam cam = make_cam(p.K, p.dist);
    const double *__restrict__ p3 = p.points3d, *__restrict__ p2 = p.points2d;
    const double thr2 = p.threshold * p.threshold;
    double Rh[9], th[3];
    hypothesis(cam, p3, p2, M, p.seed, h, Rh, th);  // (every lane: the same values)
    if (tid == 0) scount = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < M; i += PNP_NT) {
        const int in = is_inlier(cam, Rh, th, p3 + 3 * (size_t)i, p2 + 2 * (size_t)i, thr2) ? 1 : 0;
        mask[i] = (unsigned char)in;  // (this lane reads back only the bytes it wrote)
        mine += in;
    }
    atomicAdd(&scount, mine);
    __syncthreads();
    BlockEval eval{cam, p3, p2, mask, M, tid, sh};
    double R[9], t[3], cost;
    int iters;
    const bool ok = polish(eval, Rh, th, R, t, cost, iters);
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) {
            res.R[k] = ok ? R[k] : Rh[k];
            res.R_hyp[k] = Rh[k];
        }
        for (int k = 0; k < 3; ++k) {
            res.t[k] = ok ? t[k] : th[k];
            res.t_hyp[k] = th[k];
        }
        res.cost = cost;
        res.num_inliers = scount;
        res.best_h = (int)h;
        res.status = ok ? FMPNP_PNP_OK : FMPNP_PNP_POLISH_FAILED;
        res.polish_iters = iters;
    }
}

}  // namespace
}  // namespace fmpnp

using namespace fmpnp;

namespace {

// validation shared by the HIP entry points; *max_iters: the largest iters among the problems with M >= 4
int pnp_args(const fmpnp_pnp_problem *probs, int n, size_t mask_bytes, int *max_iters) {
    *max_iters = 0;
    for (int i = 0; i < n; ++i) {
        const fmpnp_pnp_problem &p = probs[i];
        if (p.M < 0 || p.iters < 1 || p.n_dist != 4 || !(p.threshold >= 0.0)) return FMPNP_EINVAL;
        if (p.M < 4) continue;
        if (!p.points3d || !p.points2d) return FMPNP_EINVAL;
        if (p.mask_offset < 0 || (unsigned long long)p.mask_offset + (unsigned long long)p.M > mask_bytes)
            return FMPNP_EINVAL;
        *max_iters = std::max(*max_iters, p.iters);
    }
    return 0;
}

}  // namespace

extern "C" {

size_t fmpnp_pnp_workspace_size(int n) { return n > 0 ? (size_t)n * sizeof(unsigned long long) : 0; }

int fmpnp_pnp_ransac_async(const fmpnp_pnp_problem *probs_dev, const fmpnp_pnp_problem *probs_host, int n,
                           fmpnp_pnp_result *results_dev, unsigned char *mask_dev, size_t mask_bytes,
                           void *workspace, size_t workspace_bytes, void *hip_stream) {
    if (n < 0) return FMPNP_EINVAL;
    if (n == 0) return 0;
    if (n > 65535) return FMPNP_ETOOBIG;
    if (!probs_dev || !probs_host || !results_dev) return FMPNP_EINVAL;
    if (!workspace || workspace_bytes < fmpnp_pnp_workspace_size(n) || ((uintptr_t)workspace & 7)) return FMPNP_EINVAL;
    int max_iters = 0;
    const int rc = pnp_args(probs_host, n, mask_dev ? mask_bytes : 0, &max_iters);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    unsigned long long *keys = (unsigned long long *)workspace;
    hipError_t e = hipMemsetAsync(keys, 0, (size_t)n * sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    if (max_iters > 0) {
        const unsigned gx = (unsigned)(((long long)max_iters + PNP_NT - 1) / PNP_NT);
        hipLaunchKernelGGL(pnp_hyp_kernel, dim3(gx, (unsigned)n), dim3(PNP_NT), 0, s, probs_dev, keys);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(pnp_finalise_kernel, dim3((unsigned)n), dim3(PNP_NT), 0, s, probs_dev, keys, results_dev,
                       mask_dev);
    return (int)hipGetLastError();
}

int fmpnp_pnp_ransac(const fmpnp_pnp_problem *probs_host, int n, int points_on_device, fmpnp_pnp_result *results,
                     unsigned char *mask, size_t mask_bytes, void *hip_stream) {
    if (n < 0) return FMPNP_EINVAL;
    if (n == 0) return 0;
    if (n > 65535) return FMPNP_ETOOBIG;
    if (!probs_host || !results) return FMPNP_EINVAL;
    int max_iters = 0;
    const int rc0 = pnp_args(probs_host, n, mask ? mask_bytes : 0, &max_iters);
    if (rc0) return rc0;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t b_probs = align256(sizeof(fmpnp_pnp_problem) * (size_t)n), b_res = align256(sizeof(fmpnp_pnp_result) * (size_t)n);
    const size_t b_keys = align256(fmpnp_pnp_workspace_size(n)), b_mask = align256(mask ? mask_bytes : 0);
    size_t b_pts = 0;
    if (!points_on_device)
        for (int i = 0; i < n; ++i)
            if (probs_host[i].M >= 4) b_pts += align256(5 * sizeof(double) * (size_t)probs_host[i].M);
    const size_t b_stage = b_probs + b_pts;  // one upload: the descriptors, then the points
    SyncCall call(SCRATCH_PNP, s, b_stage + b_res + b_keys + b_mask, b_stage);
    if (call.error()) return call.error();
    unsigned char *d_stage = call.dev, *h_stage = call.host;
    fmpnp_pnp_result *d_res = (fmpnp_pnp_result *)(d_stage + b_stage);
    unsigned char *d_keys = d_stage + b_stage + b_res, *d_mask = d_stage + b_stage + b_res + b_keys;
    fmpnp_pnp_problem *hp = (fmpnp_pnp_problem *)h_stage;
    memcpy(hp, probs_host, sizeof(fmpnp_pnp_problem) * (size_t)n);
    if (!points_on_device) {
        size_t at = b_probs;
        for (int i = 0; i < n; ++i) {
            const size_t M = (size_t)probs_host[i].M;
            if (M < 4) continue;
            memcpy(h_stage + at, probs_host[i].points3d, 3 * sizeof(double) * M);
            memcpy(h_stage + at + 3 * sizeof(double) * M, probs_host[i].points2d, 2 * sizeof(double) * M);
            hp[i].points3d = (const double *)(d_stage + at);
            hp[i].points2d = (const double *)(d_stage + at + 3 * sizeof(double) * M);
            at += align256(5 * sizeof(double) * M);
        }
    }
    hipError_t e = hipMemcpyAsync(d_stage, h_stage, b_stage, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_res, 0, b_res + b_keys + b_mask, s);
    if (e != hipSuccess) return (int)e;
    const int rc = fmpnp_pnp_ransac_async((const fmpnp_pnp_problem *)d_stage, probs_host, n, d_res,
                                          mask ? d_mask : nullptr, mask ? mask_bytes : 0, d_keys, b_keys, hip_stream);
    if (rc) return rc;
    e = hipMemcpyAsync(results, d_res, sizeof(fmpnp_pnp_result) * (size_t)n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && mask && mask_bytes) e = hipMemcpyAsync(mask, d_mask, mask_bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    return call.finish();
}

}  // extern "C"
