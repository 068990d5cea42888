// fmpnp_localize_impl.h -- the arithmetic and the decisions of the localisation chain's two glue steps
// (include/fmpnp.h states the contract), shared by the kernels of fmpnp_localize.hip and the CPU twins of
// fmpnp_localize_cpu.cpp: both call these functions for every value they write and neither unit is compiled
// with contraction, so the two agree bit for bit.  The units differ only in how they find a row's place in
// the compacted list (a ballot and a running base on the GPU, a counter on the host).  Plain C++ (the
// twin is built by the host compiler), __host__ __device__ under hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fmpnp.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FMPNP_LOC_HD __host__ __device__ inline
#else
#define FMPNP_LOC_HD inline
#endif

namespace fmpnp {
namespace loc {

constexpr int MAX_PAIRS = 65535;  // the PnP stage's grid

// exhaustive_search.py:18-19,51-54: the argmax cell's centre in image space, every fp32 operation on its own
FMPNP_LOC_HD void query_point(const fmpnp_loc_pair &p, int argmax, float out[2]) {
    const int height = p.dim[1];
    const int a[2] = {argmax % height, argmax / height};
    for (int k = 0; k < 2; ++k) {
        const float cell = p.image_shape[k] / (float)p.dim[k];
        const float scaled = (float)a[k] * cell;
        const float half = cell / 2.0f;
        out[k] = scaled + half;
    }
}

// row i of the pair (relative to its row_offset) becomes its match m
FMPNP_LOC_HD void write_match(const fmpnp_loc_pair &p, const int *argmax, const fmpnp_loc_matches &o, int i, int m) {
    const size_t d = (size_t)p.row_offset + (size_t)m;
    float q[2];
    query_point(p, argmax[(size_t)p.row_offset + (size_t)i], q);
    for (int k = 0; k < 2; ++k) {
        o.query2d_f32[2 * d + k] = q[k];
        o.query2d[2 * d + k] = (double)q[k];
        o.ref2d[2 * d + k] = p.points2d[2 * (size_t)i + k];
    }
    for (int k = 0; k < 3; ++k) o.points3d[3 * d + k] = p.points3d[3 * (size_t)i + k];
    o.src_row[d] = i;
}

// the pair's PnP problem, every byte of it
FMPNP_LOC_HD void write_problem(const fmpnp_loc_pair &p, const fmpnp_loc_params &prm, const fmpnp_loc_matches &o,
                                int count, fmpnp_pnp_problem &out) {
    out.points3d = o.points3d + 3 * (size_t)p.row_offset;
    out.points2d = o.query2d + 2 * (size_t)p.row_offset;
    for (int k = 0; k < 9; ++k) out.K[k] = p.K[k];
    for (int k = 0; k < 4; ++k) out.dist[k] = p.dist[k];
    out.threshold = prm.threshold;
    out.seed = prm.seed;
    out.mask_offset = p.row_offset;
    out.M = count > prm.minimum_matches ? count : 0;  // solve_pnp.py:44
    out.iters = prm.iters;
    out.n_dist = 4;
    out.reserved = 0;
}

// a pair's standing in its query's choice: its score, or -1 when it is absent
FMPNP_LOC_HD int pair_score(const fmpnp_loc_pair &p, const fmpnp_loc_params &prm, const fmpnp_pnp_result &r, int *kind) {
    if (r.status == FMPNP_PNP_OK && r.num_inliers >= prm.minimum_inliers) {
        *kind = FMPNP_LOC_SOLVED;
        return r.num_inliers;
    }
    if (p.has_fallback) {  // sparse_to_dense_predictor.py:179-189
        *kind = FMPNP_LOC_FALLBACK;
        return 0;
    }
    *kind = FMPNP_LOC_NONE;
    return -1;
}

// the query's best pair (predictor.py:51: the maximum score, the lowest j among equals); -1: none
FMPNP_LOC_HD int pick_best(const fmpnp_loc_pair *pairs, const fmpnp_loc_query &q, const fmpnp_loc_params &prm,
                           const fmpnp_pnp_result *results, int *best_kind) {
    int best = -1, best_score = -1;
    *best_kind = FMPNP_LOC_NONE;
    for (int j = 0; j < q.pair_count; ++j) {
        int kind;
        const int score = pair_score(pairs[q.pair_begin + j], prm, results[q.pair_begin + j], &kind);
        if (score > best_score) {
            best = j;
            best_score = score;
            *best_kind = kind;
        }
    }
    return best;
}

// the query's record, every byte of it; N: the rows the refiner's arrays get
FMPNP_LOC_HD void write_record(const fmpnp_loc_pair *pairs, const fmpnp_loc_query &q, const fmpnp_loc_params &prm,
                               const fmpnp_pnp_result *results, const int *counts, int best, int kind,
                               fmpnp_loc_record &rec) {
    const bool some = best >= 0;
    const int g = some ? q.pair_begin + best : 0;
    const bool solved = kind == FMPNP_LOC_SOLVED;
    for (int k = 0; k < 9; ++k) rec.R0[k] = !some ? 0.0 : solved ? results[g].R[k] : pairs[g].fallback_R[k];
    for (int k = 0; k < 3; ++k) rec.t0[k] = !some ? 0.0 : solved ? results[g].t[k] : pairs[g].fallback_t[k];
    rec.best = best;
    rec.kind = kind;
    rec.num_matches = some ? counts[g] : 0;
    rec.num_inliers = solved ? results[g].num_inliers : 0;
    rec.N = !some ? 0 : (solved && prm.return_masked) ? results[g].num_inliers : counts[g];
    rec.reserved = 0;
}

// match m of the best pair becomes row d of the refiner's arrays
FMPNP_LOC_HD void write_best_row(const fmpnp_loc_pair &p, const fmpnp_loc_query &q, const fmpnp_loc_matches &m_,
                                 const fmpnp_loc_best &o, int m, int d) {
    const size_t s = (size_t)p.row_offset + (size_t)m, t = (size_t)q.out_offset + (size_t)d;
    for (int k = 0; k < 3; ++k) o.pts3d[3 * t + k] = m_.points3d[3 * s + k];
    for (int k = 0; k < 2; ++k) {
        o.ref2d[2 * t + k] = m_.ref2d[2 * s + k];
        o.query2d[2 * t + k] = m_.query2d_f32[2 * s + k];
    }
}

inline bool loc_null(const fmpnp_loc_matches *m) {
    return !m || !m->query2d_f32 || !m->query2d || !m->points3d || !m->ref2d || !m->src_row || !m->counts;
}
inline bool loc_null(const fmpnp_loc_best *b) {
    return !b || !b->pts3d || !b->ref2d || !b->query2d || !b->idx || !b->records;
}

// host validation shared by the HIP entry point and the twins (the descriptors in HOST memory)
inline int pairs_args(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_params *prm, long long total_rows) {
    if (n_pairs < 0 || total_rows < 0) return FMPNP_EINVAL;
    if (n_pairs > MAX_PAIRS) return FMPNP_ETOOBIG;
    if (!prm || (n_pairs && !pairs)) return FMPNP_EINVAL;
    if (prm->iters < 1 || !(prm->threshold >= 0.0)) return FMPNP_EINVAL;
    for (int i = 0; i < n_pairs; ++i) {
        const fmpnp_loc_pair &p = pairs[i];
        if (p.n_rows < 0 || p.row_offset < 0 || p.row_offset + (long long)p.n_rows > total_rows) return FMPNP_EINVAL;
        if (p.dim[0] < 1 || p.dim[1] < 1) return FMPNP_EINVAL;
        if (p.n_rows && (!p.points3d || !p.points2d)) return FMPNP_EINVAL;
    }
    return 0;
}

inline int queries_args(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_query *queries, int n_queries,
                        long long total_rows) {
    if (n_queries < 0) return FMPNP_EINVAL;
    if (n_queries && !queries) return FMPNP_EINVAL;
    for (int i = 0; i < n_queries; ++i) {
        const fmpnp_loc_query &q = queries[i];
        if (q.pair_begin < 0 || q.pair_count < 0 || (long long)q.pair_begin + q.pair_count > n_pairs) return FMPNP_EINVAL;
        if (q.out_offset < 0 || q.out_cap < 0 || q.out_offset + (long long)q.out_cap > total_rows) return FMPNP_EINVAL;
        for (int j = 0; j < q.pair_count; ++j)
            if (pairs[q.pair_begin + j].n_rows > q.out_cap) return FMPNP_EINVAL;
    }
    return 0;
}

}  // namespace loc
}  // namespace fmpnp
