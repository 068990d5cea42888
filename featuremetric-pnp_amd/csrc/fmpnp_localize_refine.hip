// fmpnp_localize_refine.hip -- the batched refinement stage of the localisation chain on gfx950 (include/fmpnp.h,
// "batched refinement of the chain's winners"): after loc_pick_kernel, with nothing downloaded, every query's
// refiner problem is assembled and refined on the device.
//
//   loc_refine_prep_kernel    one workgroup per query: its n_res fmpnp_problem descriptors from its record, its
//                             pairs and the per-pair table of reference maps; its error flag cleared.
//   loc_refine_gather_kernel  the reference descriptors of every query in one grid: RG_ROWS rows per workgroup,
//                             the grid sized from the largest out_cap, workgroups past the device's N exit.
//                             In a CHW map the C values of a point lie H_ref W_ref elements apart, each in its own
//                             128-byte line: consecutive lanes take consecutive channels of a row
//                             (the stores coalesce, the loads cannot), every lane issues RG_UNROLL independent
//                             loads before its first store, and the rows of all the queries share the one launch
//                             -- a single query's grid is too small to keep the memory system busy.
//   loc_refine_carry_kernel   between two levels: every query's result into its slot of the results, its pose
//                             into the next level's R0 / t0.
//
// compute_cost is fmpnp_points.hip's (launch_compute_cost_batch: the per-query kernels' bodies), the levels are
// fmpnp_refine_batch_async's.  Every value of the descriptors and rows is written by fmpnp_localize_impl.h,
// which the CPU twin shares.  No kernel here waits on another workgroup.
#include <string.h>

#include <algorithm>
#include <vector>

#include "fmpnp_internal.h"
#include "fmpnp_localize_impl.h"

namespace fmpnp {
namespace {

using namespace loc;

constexpr int RP_NT = 64;
constexpr int RG_NT = 256, RG_ROWS = 4, RG_UNROLL = 8;

__global__ __launch_bounds__(RP_NT) void loc_refine_prep_kernel(const fmpnp_loc_pair *__restrict__ pairs,
                                                                const fmpnp_loc_query *__restrict__ queries,
                                                                const fmpnp_loc_refine_source *__restrict__ src,
                                                                const fmpnp_loc_refine_map *__restrict__ maps,
                                                                fmpnp_loc_refine_params rp, RefineLevels lv,
                                                                fmpnp_loc_best best, void *fref, int elem_bytes,
                                                                fmpnp_problem *__restrict__ probs,
                                                                int *__restrict__ flags) {
    const int b = blockIdx.x, n_res = refine_n_res(lv.n_levels);
    if (threadIdx.x == 0) flags[b] = 0;
    for (int r = threadIdx.x; r < n_res; r += RP_NT)
        write_refine_problem(pairs, queries[b], best.records[b], src, maps[b], rp, lv, best, fref, elem_bytes, r,
                             probs[(size_t)r * gridDim.x + b]);
}

template <typename Tout>
__global__ __launch_bounds__(RG_NT) void loc_refine_gather_kernel(const fmpnp_loc_query *__restrict__ queries,
                                                                  const fmpnp_loc_record *__restrict__ records,
                                                                  const fmpnp_loc_refine_source *__restrict__ src,
                                                                  fmpnp_loc_refine_params rp,
                                                                  const double *__restrict__ ref2d,
                                                                  Tout *__restrict__ fref, int *__restrict__ flags) {
    __shared__ int s_row[RG_ROWS], s_col[RG_ROWS];
    const fmpnp_loc_query &q = queries[blockIdx.y];
    const fmpnp_loc_record &rec = records[blockIdx.y];
    const int N = refine_count(q, rec, src), n0 = (int)blockIdx.x * RG_ROWS, tid = threadIdx.x;
    if (n0 >= N) return;  // (uniform: N = 0 without a map, so no source is read below without one)
    const fmpnp_loc_refine_source s = src[refine_pair(q, rec, src)];
    const int rows = min(RG_ROWS, N - n0);
    const size_t t0 = (size_t)q.out_offset + (size_t)n0;
    if (tid < rows) {
        int row = 0, col = 0;
        const bool ok = ref_cell(s, rp.img0, rp.img1, ref2d[2 * (t0 + tid)], ref2d[2 * (t0 + tid) + 1], &row, &col);
        s_row[tid] = ok ? row : -1;
        s_col[tid] = col;
        if (!ok) atomicOr(flags + blockIdx.y, 1);  // the reference raises IndexError here
    }
    __syncthreads();
    const int cs = rp.cstride, total = rows * cs;
    Tout *out = fref + t0 * (size_t)cs;
    for (int e0 = tid; e0 < total; e0 += RG_NT * RG_UNROLL) {
        Tout v[RG_UNROLL];
#pragma unroll
        for (int k = 0; k < RG_UNROLL; ++k) {
            const int e = e0 + k * RG_NT;
            v[k] = (Tout)0;  // (a row outside its map, and the padding channels [C, cstride))
            if (e < total) {
                const int n = e / cs, c = e - n * cs, row = s_row[n];
                if (row >= 0 && c < rp.C) v[k] = ref_value<Tout>(s, c, row, s_col[n]);
            }
        }
#pragma unroll
        for (int k = 0; k < RG_UNROLL; ++k) {
            const int e = e0 + k * RG_NT;
            if (e < total) out[e] = v[k];
        }
    }
}

// level r is done: its results (stage[n]) into results[q][r]; the next level starts from them (feature_pnp_run's
// 96-byte copy R, t -> R0, t0, over every query)
__global__ __launch_bounds__(64) void loc_refine_carry_kernel(const fmpnp_result *__restrict__ stage,
                                                              fmpnp_result *__restrict__ results, int n_res, int r,
                                                              fmpnp_problem *__restrict__ next, int n) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const fmpnp_result res = stage[b];
    results[(size_t)b * n_res + r] = res;
    if (next) {
        for (int k = 0; k < 9; ++k) next[b].R0[k] = res.R[k];
        for (int k = 0; k < 3; ++k) next[b].t0[k] = res.t[k];
    }
}

// the host descriptors of level r beside the device ones: N = the query's capacity (the plan's sizes only)
void host_level(const fmpnp_loc_query *queries, int n, const fmpnp_loc_refine_map *maps, const fmpnp_loc_refine_params &rp,
                int r, fmpnp_problem *out) {
    for (int b = 0; b < n; ++b) {
        fmpnp_problem &p = out[b];
        memset(&p, 0, sizeof(p));
        p.feat = p.fref = (const void *)(uintptr_t)256;  // (device addresses the plan never reads)
        p.pts3d = (const double *)(uintptr_t)256;
        p.Hf = maps[b].Hf;
        p.Wf = maps[b].Wf;
        p.cstride = p.ld_ref = rp.cstride;
        const bool level = rp.n_levels > 0 && r > 0;
        p.c_begin = level ? rp.levels[r - 1].c_begin : 0;
        p.c_end = level ? rp.levels[r - 1].c_end : rp.C;
        p.N = queries[b].out_cap;
        p.im_width = rp.img0;
        p.im_height = rp.img1;
    }
}

int refine_opt_args(const fmpnp_options *opt) {
    if (!opt || opt->mode != FMPNP_MODE_FORWARD || opt->layout != FMPNP_LAYOUT_FGRAD) return FMPNP_EINVAL;
    if (opt->dtype != FMPNP_F32 && opt->dtype != FMPNP_F64) return FMPNP_EINVAL;
    return 0;
}

// the LM workspace of the largest level's plan; 0 and *rc set when a plan fails
size_t lm_workspace(const fmpnp_loc_query *queries, int n, const fmpnp_loc_refine_map *maps,
                    const fmpnp_loc_refine_params &rp, const fmpnp_options *opt, std::vector<fmpnp_problem> *hd, int *rc) {
    const int n_res = refine_n_res(rp.n_levels);
    hd->resize((size_t)n_res * (size_t)std::max(n, 1));
    size_t ws = 0;
    *rc = 0;
    for (int r = 0; r < n_res; ++r) {
        fmpnp_problem *h = hd->data() + (size_t)r * n;
        host_level(queries, n, maps, rp, r, h);
        if (rp.n_levels > 0 && r == 0) continue;  // (compute_cost: point costs and one reduction, no LM launch)
        fmpnp_launch_info info;
        *rc = fmpnp_plan(h, n, opt, &info);
        if (*rc) return 0;
        ws = std::max(ws, fmpnp_workspace_size(h, n, opt));
    }
    return align256(ws);
}

}  // namespace

int localize_refine_workspace(const fmpnp_loc_query *queries_host, int n_queries, const fmpnp_loc_refine_map *maps_host,
                              const fmpnp_loc_refine_params *params, const fmpnp_options *opt, size_t *bytes) {
    *bytes = 0;
    int rc = loc::refine_args(queries_host, n_queries, maps_host, params);
    if (rc) return rc;
    rc = refine_opt_args(opt);
    if (rc || n_queries == 0) return rc;
    std::vector<fmpnp_problem> hd;
    const size_t ws = lm_workspace(queries_host, n_queries, maps_host, *params, opt, &hd, &rc);
    if (rc) return rc;
    *bytes = ws + (params->n_levels > 0 ? align256(sizeof(fmpnp_result) * (size_t)n_queries) : 0);
    return 0;
}

}  // namespace fmpnp

using namespace fmpnp;

extern "C" {

size_t fmpnp_localize_refine_workspace_size(const fmpnp_loc_query *queries_host, int n_queries,
                                            const fmpnp_loc_refine_map *maps_host,
                                            const fmpnp_loc_refine_params *params, const fmpnp_options *opt) {
    size_t bytes = 0;
    return localize_refine_workspace(queries_host, n_queries, maps_host, params, opt, &bytes) ? 0 : bytes;
}

int fmpnp_localize_refine_async(const fmpnp_loc_pair *pairs_dev, int n_pairs, const fmpnp_loc_query *queries_dev,
                                const fmpnp_loc_query *queries_host, int n_queries,
                                const fmpnp_loc_refine_source *sources_dev, const fmpnp_loc_refine_map *maps_dev,
                                const fmpnp_loc_refine_map *maps_host, const fmpnp_loc_refine_params *params,
                                const fmpnp_options *opt, const fmpnp_loc_best *best,
                                const fmpnp_loc_refine_buffers *buffers, void *workspace, size_t workspace_bytes,
                                void *hip_stream) {
    int rc = loc::refine_args(queries_host, n_queries, maps_host, params);
    if (rc) return rc;
    rc = refine_opt_args(opt);
    if (rc) return rc;
    if (n_queries == 0) return 0;
    if (n_pairs < 0 || n_pairs > loc::MAX_PAIRS || n_queries > loc::MAX_PAIRS) return n_pairs < 0 ? FMPNP_EINVAL : FMPNP_ETOOBIG;
    if (!queries_dev || !maps_dev || loc::loc_null(best) || !buffers || (n_pairs && (!pairs_dev || !sources_dev)))
        return FMPNP_EINVAL;
    if (!buffers->probs || !buffers->fref || !buffers->results || !buffers->flags) return FMPNP_EINVAL;
    const int n_levels = params->n_levels, n_res = loc::refine_n_res(n_levels), B = n_queries;
    if (n_levels > 0 && (!buffers->cost || !buffers->supported)) return FMPNP_EINVAL;
    int max_cap = 0;
    for (int b = 0; b < B; ++b) {
        if ((long long)queries_host[b].pair_begin + queries_host[b].pair_count > n_pairs) return FMPNP_EINVAL;
        max_cap = std::max(max_cap, queries_host[b].out_cap);
    }
    std::vector<fmpnp_problem> hd;
    const size_t ws = lm_workspace(queries_host, B, maps_host, *params, opt, &hd, &rc);
    if (rc) return rc;  // (FMPNP_ETOOBIG: a capacity the LM plan cannot take)
    const size_t b_stage = n_levels > 0 ? align256(sizeof(fmpnp_result) * (size_t)B) : 0;
    if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < ws + b_stage) return FMPNP_EINVAL;
    fmpnp_result *stage = (fmpnp_result *)((unsigned char *)workspace + ws);
    hipStream_t s = (hipStream_t)hip_stream;
    const int es = opt->dtype == FMPNP_F64 ? 8 : 4;
    const loc::RefineLevels lv = loc::refine_levels(*params);
    fmpnp_loc_refine_params rp = *params;
    rp.levels = nullptr;  // (a host pointer: the kernels take the levels by value)
    hipLaunchKernelGGL(loc_refine_prep_kernel, dim3((unsigned)B), dim3(RP_NT), 0, s, pairs_dev, queries_dev, sources_dev,
                       maps_dev, rp, lv, *best, buffers->fref, es, buffers->probs, buffers->flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (max_cap > 0) {
        const dim3 grid((unsigned)((max_cap + RG_ROWS - 1) / RG_ROWS), (unsigned)B);
        if (opt->dtype == FMPNP_F64)
            hipLaunchKernelGGL(loc_refine_gather_kernel<double>, grid, dim3(RG_NT), 0, s, queries_dev,
                               (const fmpnp_loc_record *)best->records, sources_dev, rp, (const double *)best->ref2d,
                               (double *)buffers->fref, buffers->flags);
        else
            hipLaunchKernelGGL(loc_refine_gather_kernel<float>, grid, dim3(RG_NT), 0, s, queries_dev,
                               (const fmpnp_loc_record *)best->records, sources_dev, rp, (const double *)best->ref2d,
                               (float *)buffers->fref, buffers->flags);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (n_levels > 0) {
        static_assert(offsetof(fmpnp_loc_query, out_offset) == 0, "the queries' out_offset leads the descriptor");
        e = launch_compute_cost_batch(buffers->probs, B, max_cap, (const long long *)queries_dev, sizeof(fmpnp_loc_query),
                                      opt->layout, opt->dtype, opt->use_ratio, opt->ratio_threshold, buffers->cost,
                                      buffers->supported, buffers->results, n_res, s);
        if (e != hipSuccess) return (int)e;
    }
    for (int r = n_levels > 0 ? 1 : 0; r < n_res; ++r) {
        fmpnp_result *target = n_levels > 0 ? stage : buffers->results;
        rc = fmpnp_refine_batch_async(buffers->probs + (size_t)r * B, hd.data() + (size_t)r * B, B, max_cap, opt, target,
                                      nullptr, 0, workspace, ws, hip_stream);
        if (rc) return rc;
        if (n_levels > 0) {
            fmpnp_problem *next = r + 1 < n_res ? buffers->probs + (size_t)(r + 1) * B : nullptr;
            hipLaunchKernelGGL(loc_refine_carry_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s,
                               (const fmpnp_result *)stage, buffers->results, n_res, r, next, B);
            e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
    }
    return 0;
}

}  // extern "C"
