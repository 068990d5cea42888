// fmpnp_localize.hip -- the two glue kernels of the localisation chain on gfx950 (include/fmpnp.h,
// "localisation chain"; s2dhm/pose_prediction/sparse_to_dense_predictor.py:140-191,233-244, predictor.py:48-73).
//
//   loc_build_kernel  one 256-lane workgroup per pair: the rows that passed the ratio test become the pair's
//                     PnP problem, in ascending order, and the problem's descriptor is written in device
//                     memory (the PnP kernels read M and the point pointers from there only).
//   loc_pick_kernel   one 256-lane workgroup per query: the best pair of the PnP results, its record and the
//                     refiner's arrays, compacted in ascending order.
//
// Both compact the same way: a tile of 256 rows per round, each wave's ballot gives a lane its place among
// the wave's kept rows, the four waves' totals meet in LDS, and a running base carries the place across the
// tiles -- any n_rows, ordered output, no atomics.  Every value is written by fmpnp_localize_impl.h, which
// the CPU twins share.
#include <string.h>

#include <algorithm>
#include <vector>

#include "fmpnp_internal.h"
#include "fmpnp_localize_impl.h"

namespace fmpnp {
namespace {

using namespace loc;

constexpr int LOC_NT = 256;
constexpr int LOC_WAVES = LOC_NT / 64;

// the place of this lane's kept row among the tile's kept rows, and the tile's total (every lane calls it)
__device__ __forceinline__ int tile_place(bool keep, int *wsum, int *total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long b = __ballot(keep);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int before = 0, sum = 0;
    for (int k = 0; k < LOC_WAVES; ++k) {
        const int c = wsum[k];
        before += k < w ? c : 0;
        sum += c;
    }
    __syncthreads();  // (the next tile overwrites wsum)
    *total = sum;
    return before + pre;
}

__global__ __launch_bounds__(LOC_NT) void loc_build_kernel(const fmpnp_loc_pair *__restrict__ pairs,
                                                           fmpnp_loc_params prm, const int *__restrict__ argmax,
                                                           const unsigned char *__restrict__ mask,
                                                           fmpnp_loc_matches out, fmpnp_pnp_problem *__restrict__ probs) {
    __shared__ int wsum[LOC_WAVES];
    const fmpnp_loc_pair &p = pairs[blockIdx.x];
    const int n_rows = p.n_rows, tid = threadIdx.x;
    const unsigned char *m = mask + p.row_offset;
    int base = 0;
    for (int t0 = 0; t0 < n_rows; t0 += LOC_NT) {  // (uniform trip count: the barriers inside are safe)
        const int i = t0 + tid;
        const bool keep = i < n_rows && m[i] != 0;
        int total;
        const int place = tile_place(keep, wsum, &total);
        if (keep) write_match(p, argmax, out, i, base + place);
        base += total;
    }
    if (tid == 0) {
        out.counts[blockIdx.x] = base;
        write_problem(p, prm, out, base, probs[blockIdx.x]);
    }
}

__global__ __launch_bounds__(LOC_NT) void loc_pick_kernel(const fmpnp_loc_pair *__restrict__ pairs,
                                                          const fmpnp_loc_query *__restrict__ queries,
                                                          fmpnp_loc_params prm,
                                                          const fmpnp_pnp_result *__restrict__ results,
                                                          const unsigned char *__restrict__ pnp_mask,
                                                          fmpnp_loc_matches mt, fmpnp_loc_best out) {
    __shared__ int wsum[LOC_WAVES];
    const fmpnp_loc_query &q = queries[blockIdx.x];
    const int tid = threadIdx.x;
    int kind;
    const int best = pick_best(pairs, q, prm, results, &kind);  // (every lane: the same few loads)
    if (tid == 0) write_record(pairs, q, prm, results, mt.counts, best, kind, out.records[blockIdx.x]);
    if (best < 0) return;  // (uniform)
    const fmpnp_loc_pair &p = pairs[q.pair_begin + best];
    const int count = mt.counts[q.pair_begin + best];
    if (kind == FMPNP_LOC_FALLBACK) {
        for (int m = tid; m < count; m += LOC_NT) write_best_row(p, q, mt, out, m, m);
        return;
    }
    const bool masked = prm.return_masked != 0;
    const unsigned char *inl = pnp_mask + p.row_offset;  // (count > minimum_matches here: M = count bytes written)
    int base = 0;
    for (int t0 = 0; t0 < count; t0 += LOC_NT) {
        const int m = t0 + tid;
        const bool keep = m < count && inl[m] != 0;
        int total;
        const int place = tile_place(keep, wsum, &total);
        if (keep) out.idx[(size_t)q.out_offset + (size_t)(base + place)] = m;
        if (masked) {
            if (keep) write_best_row(p, q, mt, out, m, base + place);
        } else if (m < count) {
            write_best_row(p, q, mt, out, m, m);
        }
        base += total;
    }
}

}  // namespace
}  // namespace fmpnp

using namespace fmpnp;

static int localize_run(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                        const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k, int n_queries,
                        int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                        const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                        unsigned char *pnp_mask, int match_precision, const LocalizeRefine *rf,
                        const fmpnp_loc_query_layers *ql, void *hip_stream);

extern "C" {

size_t fmpnp_localize_workspace_size(int n_pairs) {
    if (n_pairs <= 0) return 0;
    const size_t probs = align256(sizeof(fmpnp_pnp_problem) * (size_t)n_pairs);
    return probs + fmpnp_pnp_workspace_size(n_pairs);
}

int fmpnp_localize_async(const fmpnp_loc_pair *pairs_dev, const fmpnp_loc_pair *pairs_host, int n_pairs,
                         const fmpnp_loc_query *queries_dev, const fmpnp_loc_query *queries_host, int n_queries,
                         const fmpnp_loc_params *params, const int *argmax, const unsigned char *mask,
                         long long total_rows, const fmpnp_loc_matches *matches, const fmpnp_loc_best *best,
                         fmpnp_pnp_result *results_dev, unsigned char *pnp_mask_dev, void *workspace,
                         size_t workspace_bytes, void *hip_stream) {
    int rc = loc::pairs_args(pairs_host, n_pairs, params, total_rows);
    if (rc) return rc;
    rc = loc::queries_args(pairs_host, n_pairs, queries_host, n_queries, total_rows);
    if (rc) return rc;
    if (loc::loc_null(matches) || loc::loc_null(best)) return FMPNP_EINVAL;
    if (n_queries && !queries_dev) return FMPNP_EINVAL;
    if (n_pairs) {
        if (!pairs_dev || !results_dev) return FMPNP_EINVAL;
        if (total_rows && (!argmax || !mask || !pnp_mask_dev)) return FMPNP_EINVAL;
        if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < fmpnp_localize_workspace_size(n_pairs))
            return FMPNP_EINVAL;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    if (n_pairs) {
        fmpnp_pnp_problem *probs_dev = (fmpnp_pnp_problem *)workspace;
        const size_t b_probs = align256(sizeof(fmpnp_pnp_problem) * (size_t)n_pairs);
        hipLaunchKernelGGL(loc_build_kernel, dim3((unsigned)n_pairs), dim3(LOC_NT), 0, s, pairs_dev, *params, argmax, mask,
                           *matches, probs_dev);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        // the host descriptors beside the device ones: M = the capacity, for validation and the grid only
        std::vector<fmpnp_pnp_problem> host((size_t)n_pairs);
        for (int i = 0; i < n_pairs; ++i) {
            loc::write_problem(pairs_host[i], *params, *matches, pairs_host[i].n_rows, host[i]);
            host[i].M = pairs_host[i].n_rows;
        }
        rc = fmpnp_pnp_ransac_async(probs_dev, host.data(), n_pairs, results_dev, pnp_mask_dev, (size_t)total_rows,
                                    (unsigned char *)workspace + b_probs, workspace_bytes - b_probs, hip_stream);
        if (rc) return rc;
    }
    if (n_queries) {
        hipLaunchKernelGGL(loc_pick_kernel, dim3((unsigned)n_queries), dim3(LOC_NT), 0, s, pairs_dev, queries_dev, *params,
                           results_dev, pnp_mask_dev, *matches, *best);
        return (int)hipGetLastError();
    }
    return 0;
}

int fmpnp_localize(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                   const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k, int n_queries, int C,
                   double ratio, const fmpnp_loc_params *params, long long total_rows, const fmpnp_loc_best *best,
                   const fmpnp_loc_matches *all, fmpnp_pnp_result *results, unsigned char *pnp_mask, void *hip_stream) {
    return fmpnp_localize_ex(pairs, sources, n_pairs, queries, query_dense, top_k, n_queries, C, ratio, params, total_rows,
                             best, all, results, pnp_mask, FMPNP_MATCH_F32, hip_stream);
}

int fmpnp_localize_ex(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                      const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k, int n_queries,
                      int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                      const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                      unsigned char *pnp_mask, int match_precision, void *hip_stream) {
    return localize_run(pairs, sources, n_pairs, queries, query_dense, top_k, n_queries, C, ratio, params, total_rows, best,
                        all, results, pnp_mask, match_precision, nullptr, nullptr, hip_stream);
}

int fmpnp_localize_layers(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                          const fmpnp_loc_query *queries, const fmpnp_loc_query_layers *query_layers, const int *top_k,
                          int n_queries, int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                          const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                          unsigned char *pnp_mask, void *hip_stream) {
    if (n_queries > 0 && !query_layers) return FMPNP_EINVAL;
    return localize_run(pairs, sources, n_pairs, queries, nullptr, top_k, n_queries, C, ratio, params, total_rows, best, all,
                        results, pnp_mask, FMPNP_MATCH_F32, nullptr, query_layers, hip_stream);
}

int fmpnp_localize_refined(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                           const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k,
                           int n_queries, int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                           const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                           unsigned char *pnp_mask, int match_precision,
                           const fmpnp_loc_refine_source *refine_sources, const int *query_hw,
                           const fmpnp_loc_refine_params *refine_params, const fmpnp_options *opt,
                           fmpnp_result *refine_results, int *refine_flags, void *hip_stream) {
    if (!refine_params || !opt || (n_pairs > 0 && !refine_sources)) return FMPNP_EINVAL;
    if (n_queries > 0 && (!query_hw || !refine_results || !refine_flags)) return FMPNP_EINVAL;
    const LocalizeRefine rf{refine_sources, query_hw, refine_params, opt, refine_results, refine_flags};
    return localize_run(pairs, sources, n_pairs, queries, query_dense, top_k, n_queries, C, ratio, params, total_rows, best,
                        all, results, pnp_mask, match_precision, &rf, nullptr, hip_stream);
}

}  // extern "C"

// the body of fmpnp_localize_ex and fmpnp_localize_refined (rf: NULL, or the refinement stage queued behind the
// pick; every size it adds is 0 without it, so the chain's carve and download are then unchanged)
static int localize_run(const fmpnp_loc_pair *pairs, const fmpnp_loc_source *sources, int n_pairs,
                        const fmpnp_loc_query *queries, const float *const *query_dense, const int *top_k, int n_queries,
                        int C, double ratio, const fmpnp_loc_params *params, long long total_rows,
                        const fmpnp_loc_best *best, const fmpnp_loc_matches *all, fmpnp_pnp_result *results,
                        unsigned char *pnp_mask, int match_precision, const LocalizeRefine *rf,
                        const fmpnp_loc_query_layers *ql, void *hip_stream) {
    if (match_precision != FMPNP_MATCH_F32 && match_precision != FMPNP_MATCH_F16) return FMPNP_EINVAL;
    int rc = loc::pairs_args(pairs, n_pairs, params, total_rows);
    if (rc) return rc;
    rc = loc::queries_args(pairs, n_pairs, queries, n_queries, total_rows);
    if (rc) return rc;
    if (loc::loc_null(best) || (all && loc::loc_null(all)) || C < 1) return FMPNP_EINVAL;
    if (n_pairs && !sources) return FMPNP_EINVAL;
    if (n_queries && ((!query_dense && !ql) || !top_k)) return FMPNP_EINVAL;
    if (ql && (rf || match_precision != FMPNP_MATCH_F32)) return FMPNP_EINVAL;  // (both read dense query maps)
    size_t out_rows = 0;
    for (int q = 0; q < n_queries; ++q) {
        out_rows = std::max(out_rows, (size_t)(queries[q].out_offset + queries[q].out_cap));
        if (ql && queries[q].pair_count) {  // (the layers' own checks: the match call's; here what ties them to the pairs)
            const fmpnp_loc_pair &f = pairs[queries[q].pair_begin];
            if (ql[q].H < 1 || ql[q].W < 1 || (long long)ql[q].H * ql[q].W != (long long)f.dim[0] * f.dim[1])
                return FMPNP_EINVAL;
            if (!ql[q].layers || ql[q].L < 1 || ql[q].L > 8) return FMPNP_EINVAL;
            long long channels = 0;
            for (int l = 0; l < ql[q].L; ++l) channels += ql[q].layers[l].C;
            if (channels != C) return FMPNP_EINVAL;  // (the rows are [C]: no column may go unread)
        }
        if (!ql && queries[q].pair_count && !query_dense[q]) return FMPNP_EINVAL;
        for (int j = 1; j < queries[q].pair_count; ++j) {  // (one match call per query: its pairs' rows are contiguous)
            const fmpnp_loc_pair &a = pairs[queries[q].pair_begin + j - 1], &b = pairs[queries[q].pair_begin + j];
            if (b.row_offset != a.row_offset + a.n_rows || b.dim[0] != a.dim[0] || b.dim[1] != a.dim[1]) return FMPNP_EINVAL;
        }
    }
    for (int g = 0; g < n_pairs; ++g) {
        const fmpnp_loc_source &src = sources[g];
        if (!pairs[g].n_rows) continue;
        if (!src.dense_chw && (!src.sparse || src.ld_sparse < C)) return FMPNP_EINVAL;
        if (src.dense_chw && (src.D1 < 1 || src.D2 < 1)) return FMPNP_EINVAL;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t T = (size_t)total_rows, P = (size_t)n_pairs, Q = (size_t)n_queries, O = out_rows;
    const bool every = all || results || pnp_mask;
    // the refinement stage: its host-side tables and sizes (all 0 without it)
    std::vector<fmpnp_loc_refine_map> rmaps;
    size_t r_res = 0, r_flag = 0, r_probs = 0, r_fref = 0, r_cost = 0, r_sup = 0, r_ws = 0, r_src = 0, r_maps = 0;
    int rn_res = 0, res_bytes = 4;
    if (rf) {
        const fmpnp_loc_refine_params &rp = *rf->params;
        if (rp.C != C || rp.cstride != (C + 3) / 4 * 4 || (rf->opt->sobel_flags & ~3)) return FMPNP_EINVAL;
        rmaps.resize(Q);
        for (int q = 0; q < n_queries; ++q) {
            rmaps[q] = fmpnp_loc_refine_map{nullptr, rf->query_hw[2 * q], rf->query_hw[2 * q + 1]};
            if (rmaps[q].Hf < 1 || rmaps[q].Wf < 1 || !query_dense[q]) return FMPNP_EINVAL;
            if (queries[q].pair_count) {  // (the match reads the same map as [C][dim[0] * dim[1]])
                const fmpnp_loc_pair &f = pairs[queries[q].pair_begin];
                if ((long long)rmaps[q].Hf * rmaps[q].Wf != (long long)f.dim[0] * f.dim[1]) return FMPNP_EINVAL;
            }
        }
        for (int g = 0; g < n_pairs; ++g) {
            const fmpnp_loc_refine_source &rs = rf->sources[g];
            if (rs.ref_chw && (rs.H_ref < 1 || rs.W_ref < 1 || (rs.dtype != FMPNP_F32 && rs.dtype != FMPNP_F64)))
                return FMPNP_EINVAL;
        }
        rc = localize_refine_workspace(queries, n_queries, rmaps.data(), rf->params, rf->opt, &r_ws);
        if (rc) return rc;  // (FMPNP_ETOOBIG: a capacity the LM plan cannot take)
        rn_res = loc::refine_n_res(rp.n_levels);
        res_bytes = rf->opt->dtype == FMPNP_F64 ? 8 : 4;
        r_res = sizeof(fmpnp_result) * Q * rn_res;
        r_flag = 4 * Q;
        r_probs = sizeof(fmpnp_problem) * Q * rn_res;
        r_fref = O * (size_t)rp.cstride * res_bytes;
        r_cost = 8 * O;
        r_sup = 4 * O;
        r_src = sizeof(fmpnp_loc_refine_source) * P;
        r_maps = sizeof(fmpnp_loc_refine_map) * Q;
    }
    // the upload: the descriptors, then every pair's points (then the refinement's tables)
    const size_t u_pairs = 0, u_q = u_pairs + align256(sizeof(fmpnp_loc_pair) * P), u_p3 = u_q + align256(sizeof(fmpnp_loc_query) * Q);
    const size_t u_p2 = u_p3 + align256(24 * T), u_rsrc = u_p2 + align256(16 * T), u_rmaps = u_rsrc + align256(r_src);
    const size_t n_up = u_rmaps + align256(r_maps);
    // the outputs in download order: (the refinement's results and flags,) the records and the best pairs' arrays,
    // then every pair's, then what stays
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += align256(bytes);
        return o;
    };
    const size_t o_rres = take(r_res), o_rflag = take(r_flag);
    const size_t o_rec = take(sizeof(fmpnp_loc_record) * Q), o_bx3 = take(24 * O), o_br2 = take(16 * O), o_bq = take(8 * O);
    const size_t o_bidx = take(4 * O), n_head = at;
    const size_t o_cnt = take(4 * P), o_res = take(sizeof(fmpnp_pnp_result) * P), o_pm = take(T), o_mq32 = take(8 * T);
    const size_t o_mx3 = take(24 * T), o_mr2 = take(16 * T), o_src = take(4 * T), n_every = at;
    const size_t o_mq64 = take(16 * T), o_arg = take(4 * T), o_top = take(4 * T), o_kth = take(4 * T), o_mask = take(T);
    const size_t b_wsl = align256(fmpnp_localize_workspace_size(n_pairs)), o_wsl = take(b_wsl), o_rows = take(4 * T * (size_t)C);
    size_t b_wsm = 0;
    for (int q = 0; q < n_queries; ++q) {
        if (!queries[q].pair_count) continue;
        const fmpnp_loc_pair &f = pairs[queries[q].pair_begin], &l = pairs[queries[q].pair_begin + queries[q].pair_count - 1];
        const long long n_q = l.row_offset + l.n_rows - f.row_offset, wh = (long long)f.dim[0] * f.dim[1];
        if (n_q > 0x7fffffffLL || wh > 0x7fffffffLL) return FMPNP_ETOOBIG;
        if (ql) {
            const size_t b = fmpnp_match_layers_workspace_size(ql[q].layers, ql[q].L, (int)n_q, ql[q].H, ql[q].W);
            if (n_q && !b) return FMPNP_EINVAL;
            b_wsm = std::max(b_wsm, align256(b));
        } else {
            b_wsm = std::max(b_wsm, align256(fmpnp_match_workspace_size_ex((int)n_q, C, (int)wh, match_precision)));
        }
    }
    const size_t o_wsm = take(b_wsm);
    // the refinement stage's device buffers, then every query's packed map
    const size_t o_rprobs = take(r_probs), o_rfref = take(r_fref), o_rcost = take(r_cost), o_rsup = take(r_sup);
    const size_t o_rws = take(r_ws);
    std::vector<size_t> o_feat(rmaps.size());
    for (size_t q = 0; q < rmaps.size(); ++q)
        o_feat[q] = take((size_t)rmaps[q].Hf * rmaps[q].Wf * 3 * (size_t)rf->params->cstride * res_bytes);
    const size_t n_dev = at, n_down = every ? n_every : n_head;
    SyncCall call(SCRATCH_LOCALIZE, s, n_up + n_dev, n_up + n_down);
    if (call.error()) return call.error();
    unsigned char *d_up = call.dev, *d_out = call.dev + n_up, *h_up = call.host, *h_down = call.host + n_up;
    fmpnp_loc_pair *hp = (fmpnp_loc_pair *)(h_up + u_pairs);
    if (P) memcpy(hp, pairs, sizeof(fmpnp_loc_pair) * P);
    if (Q) memcpy(h_up + u_q, queries, sizeof(fmpnp_loc_query) * Q);
    if (rf) {
        if (P) memcpy(h_up + u_rsrc, rf->sources, r_src);
        for (size_t q = 0; q < Q; ++q) rmaps[q].feat = d_out + o_feat[q];
        if (Q) memcpy(h_up + u_rmaps, rmaps.data(), r_maps);
    }
    for (int g = 0; g < n_pairs; ++g) {
        const size_t off = (size_t)pairs[g].row_offset, n = (size_t)pairs[g].n_rows;
        if (n) {
            memcpy(h_up + u_p3 + 24 * off, pairs[g].points3d, 24 * n);
            memcpy(h_up + u_p2 + 16 * off, pairs[g].points2d, 16 * n);
        }
        hp[g].points3d = (const double *)(d_up + u_p3 + 24 * off);
        hp[g].points2d = (const double *)(d_up + u_p2 + 16 * off);
    }
    hipError_t e = hipMemcpyAsync(d_up, h_up, n_up, hipMemcpyHostToDevice, s);
    // (a FMPNP_PNP_TOO_FEW problem writes only its status: its result and mask bytes read as zeros)
    if (e == hipSuccess && P) e = hipMemsetAsync(d_out + o_res, 0, align256(sizeof(fmpnp_pnp_result) * P) + align256(T), s);
    if (e != hipSuccess) return (int)e;
    if (rf) {
        // the queries' packs do not depend on the chain: queued ahead of the match (fmpnp_pack_features_batch's
        // launches; the Sobel pack writes channels < C, so a padded stride is zeroed first, as fmpnp_feature_pnp does)
        const int cs = rf->params->cstride, fl = rf->opt->sobel_flags;
        for (int q = 0; q < n_queries; ++q) {
            unsigned char *dst = d_out + o_feat[q];
            if (cs != C) e = hipMemsetAsync(dst, 0, (size_t)rmaps[q].Hf * rmaps[q].Wf * 3 * (size_t)cs * res_bytes, s);
            if (e == hipSuccess)
                e = launch_pack(query_dense[q], nullptr, nullptr, FMPNP_F32, C, rmaps[q].Hf, rmaps[q].Wf, dst, rf->opt->dtype,
                                cs, fl & 1, (fl >> 1) & 1, s, 3);
            if (e != hipSuccess) return (int)e;
        }
    }
    float *rows = (float *)(d_out + o_rows);
    for (int g = 0; g < n_pairs; ++g) {  // the sparse descriptors, straight into the concatenated rows
        const fmpnp_loc_source &src = sources[g];
        const size_t off = (size_t)pairs[g].row_offset, n = (size_t)pairs[g].n_rows;
        if (!n) continue;
        if (src.dense_chw) {
            rc = fmpnp_gather_sparse_descriptors(src.dense_chw, C, src.D1, src.D2, hp[g].points2d, (int)n, src.cell0, src.cell1,
                                                 rows + off * (size_t)C, C, hip_stream);
            if (rc) return rc;
        } else {
            e = hipMemcpy2DAsync(rows + off * (size_t)C, 4 * (size_t)C, src.sparse, 4 * (size_t)src.ld_sparse, 4 * (size_t)C, n,
                                 hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return (int)e;
        }
    }
    for (int q = 0; q < n_queries; ++q) {
        if (!queries[q].pair_count) continue;
        const fmpnp_loc_pair &f = pairs[queries[q].pair_begin], &l = pairs[queries[q].pair_begin + queries[q].pair_count - 1];
        const size_t r0 = (size_t)f.row_offset;
        const int n_q = (int)(l.row_offset + l.n_rows - f.row_offset), wh = f.dim[0] * f.dim[1];
        if (!n_q) continue;
        if (ql) {  // the query as its layers: the norm plane once, the rows of all its references in one call
            rc = fmpnp_exhaustive_match_layers_async(rows + r0 * (size_t)C, n_q, C, ql[q].layers, ql[q].L, ql[q].B, ql[q].item,
                                                     ql[q].H, ql[q].W, ql[q].flags, top_k[q], ratio, (int *)(d_out + o_arg) + r0,
                                                     (float *)(d_out + o_top) + r0, (float *)(d_out + o_kth) + r0,
                                                     d_out + o_mask + r0, nullptr, d_out + o_wsm, b_wsm, hip_stream);
            if (rc) return rc;
            continue;
        }
        rc = fmpnp_exhaustive_match_ex_async(rows + r0 * (size_t)C, n_q, C, query_dense[q], C, wh, wh, top_k[q], ratio,
                                             (int *)(d_out + o_arg) + r0, (float *)(d_out + o_top) + r0,
                                             (float *)(d_out + o_kth) + r0, d_out + o_mask + r0, nullptr, d_out + o_wsm,
                                             b_wsm, match_precision, hip_stream);
        if (rc) return rc;
    }
    const fmpnp_loc_matches dm{(float *)(d_out + o_mq32), (double *)(d_out + o_mq64), (double *)(d_out + o_mx3),
                               (double *)(d_out + o_mr2), (int *)(d_out + o_src), (int *)(d_out + o_cnt)};
    const fmpnp_loc_best db{(double *)(d_out + o_bx3), (double *)(d_out + o_br2), (float *)(d_out + o_bq),
                            (int *)(d_out + o_bidx), (fmpnp_loc_record *)(d_out + o_rec)};
    rc = fmpnp_localize_async((const fmpnp_loc_pair *)(d_up + u_pairs), hp, n_pairs, (const fmpnp_loc_query *)(d_up + u_q),
                              queries, n_queries, params, (const int *)(d_out + o_arg), d_out + o_mask, total_rows, &dm, &db,
                              (fmpnp_pnp_result *)(d_out + o_res), d_out + o_pm, d_out + o_wsl, b_wsl, hip_stream);
    if (rc) return rc;
    if (rf && Q) {
        const fmpnp_loc_refine_buffers rb{(fmpnp_problem *)(d_out + o_rprobs), d_out + o_rfref, (double *)(d_out + o_rcost),
                                          (int *)(d_out + o_rsup), (fmpnp_result *)(d_out + o_rres), (int *)(d_out + o_rflag)};
        rc = fmpnp_localize_refine_async((const fmpnp_loc_pair *)(d_up + u_pairs), n_pairs, (const fmpnp_loc_query *)(d_up + u_q),
                                         queries, n_queries, (const fmpnp_loc_refine_source *)(d_up + u_rsrc),
                                         (const fmpnp_loc_refine_map *)(d_up + u_rmaps), rmaps.data(), rf->params, rf->opt,
                                         &db, &rb, d_out + o_rws, r_ws, hip_stream);
        if (rc) return rc;
    }
    e = hipMemcpyAsync(h_down, d_out, n_down, hipMemcpyDeviceToHost, s);  // the one download
    if (e != hipSuccess) return (int)e;
    rc = call.finish();                                                   // the one wait
    if (rc) return rc;
    // the pinned staging -> the caller's arrays: only the rows the contract names
    const fmpnp_loc_record *rec = (const fmpnp_loc_record *)(h_down + o_rec);
    for (int q = 0; q < n_queries; ++q) {
        best->records[q] = rec[q];
        const size_t o = (size_t)queries[q].out_offset, N = (size_t)rec[q].N, ni = (size_t)rec[q].num_inliers;
        memcpy(best->pts3d + 3 * o, h_down + o_bx3 + 24 * o, 24 * N);
        memcpy(best->ref2d + 2 * o, h_down + o_br2 + 16 * o, 16 * N);
        memcpy(best->query2d + 2 * o, h_down + o_bq + 8 * o, 8 * N);
        memcpy(best->idx + o, h_down + o_bidx + 4 * o, 4 * ni);
    }
    if (rf && Q) {
        memcpy(rf->results, h_down + o_rres, r_res);
        memcpy(rf->flags, h_down + o_rflag, r_flag);
    }
    if (results && P) memcpy(results, h_down + o_res, sizeof(fmpnp_pnp_result) * P);
    if (pnp_mask && T) memcpy(pnp_mask, h_down + o_pm, T);
    if (all) {
        const int *cnt = (const int *)(h_down + o_cnt);
        for (int g = 0; g < n_pairs; ++g) {
            const size_t o = (size_t)pairs[g].row_offset, n = (size_t)cnt[g];
            all->counts[g] = cnt[g];
            memcpy(all->query2d_f32 + 2 * o, h_down + o_mq32 + 8 * o, 8 * n);
            memcpy(all->points3d + 3 * o, h_down + o_mx3 + 24 * o, 24 * n);
            memcpy(all->ref2d + 2 * o, h_down + o_mr2 + 16 * o, 16 * n);
            memcpy(all->src_row + o, h_down + o_src + 4 * o, 4 * n);
            for (size_t i = 0; i < 2 * n; ++i) all->query2d[2 * o + i] = (double)all->query2d_f32[2 * o + i];
        }
    }
    return 0;
}
