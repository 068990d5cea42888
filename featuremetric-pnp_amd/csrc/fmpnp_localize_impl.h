// fmpnp_localize_impl.h -- the arithmetic and the decisions of the localisation chain's two glue steps and of
// its batched refinement stage's prep and gather steps (include/fmpnp.h states the contract), shared by the
// kernels of fmpnp_localize.hip / fmpnp_localize_refine.hip and the CPU twins of fmpnp_localize_cpu.cpp: both
// sides call these functions for every value they write and no unit is compiled with contraction, so they agree
// bit for bit.  The units differ only in how they find a row's place in
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

// ---- the batched refinement stage (include/fmpnp.h, "batched refinement of the chain's winners") -------------

// the levels ride in the kernel's arguments
struct RefineLevels {
    int n_levels;
    fmpnp_level lv[FMPNP_LOC_REFINE_MAX_LEVELS];
};

FMPNP_LOC_HD int refine_n_res(int n_levels) { return n_levels > 0 ? n_levels + 1 : 1; }

// the pair whose reference map the query's refinement reads, or -1: kind NONE or a NULL source (then N = 0)
FMPNP_LOC_HD int refine_pair(const fmpnp_loc_query &q, const fmpnp_loc_record &rec, const fmpnp_loc_refine_source *src) {
    if (rec.kind == FMPNP_LOC_NONE || rec.best < 0 || rec.best >= q.pair_count) return -1;
    const int g = q.pair_begin + rec.best;
    return src[g].ref_chw ? g : -1;
}

// the rows the query's refinement reads: the record's N (never above the query's capacity), 0 without a map
FMPNP_LOC_HD int refine_count(const fmpnp_loc_query &q, const fmpnp_loc_record &rec, const fmpnp_loc_refine_source *src) {
    if (refine_pair(q, rec, src) < 0 || rec.N < 0) return 0;
    return rec.N < q.out_cap ? rec.N : q.out_cap;
}

// descriptor r of the query, every field of it (r = 0 with levels: compute_cost over [0, C))
FMPNP_LOC_HD void write_refine_problem(const fmpnp_loc_pair *pairs, const fmpnp_loc_query &q, const fmpnp_loc_record &rec,
                                       const fmpnp_loc_refine_source *src, const fmpnp_loc_refine_map &map,
                                       const fmpnp_loc_refine_params &rp, const RefineLevels &lv,
                                       const fmpnp_loc_best &best, const void *fref, int elem_bytes, int r,
                                       fmpnp_problem &out) {
    out.feat = map.feat;
    out.fref = (const unsigned char *)fref + (size_t)q.out_offset * (size_t)rp.cstride * (size_t)elem_bytes;
    out.pts3d = best.pts3d + 3 * (size_t)q.out_offset;
    out.Hf = map.Hf;
    out.Wf = map.Wf;
    out.cstride = rp.cstride;
    const bool level = lv.n_levels > 0 && r > 0;
    int cb = 0, ce = rp.C;
    // (a select over constant indices: the levels are kernel arguments, and a variable index would move them to scratch)
#if defined(__clang__)
#pragma unroll
#endif
    for (int l = 0; l < FMPNP_LOC_REFINE_MAX_LEVELS; ++l)
        if (level && l == r - 1) {
            cb = lv.lv[l].c_begin;
            ce = lv.lv[l].c_end;
        }
    out.c_begin = cb;
    out.c_end = ce;
    out.ld_ref = rp.cstride;
    out.N = refine_count(q, rec, src);
    out.im_width = rp.img0;
    out.im_height = rp.img1;
    // the K of the query's LAST pair (sparse_to_dense_predictor.py:143,167,244), or of the best one
    const int last = q.pair_count > 0 ? q.pair_begin + q.pair_count - 1 : -1;
    const int kp = (rp.intrinsics == FMPNP_LOC_K_BEST && rec.best >= 0 && rec.best < q.pair_count) ? q.pair_begin + rec.best : last;
    for (int k = 0; k < 9; ++k) out.K[k] = kp < 0 ? 0.0 : pairs[kp].K[k];
    for (int k = 0; k < 9; ++k) out.R0[k] = rec.R0[k];  // (a fallback winner: the fallback pose, the pick put it there)
    for (int k = 0; k < 3; ++k) out.t0[k] = rec.t0[k];
    out.window = nullptr;
}

// fmpnp_gather_reference's index of an inlier (x, y) (fmpnp_pack.hip gather_ref_kernel; optimize_feature_pnp.py:
// 51-56): truncation toward zero, python's negative-index wrap; false: outside the map or NaN (the reference's
// IndexError).  A product beyond int's range is outside whatever the conversion would make of it.
FMPNP_LOC_HD bool ref_cell(const fmpnp_loc_refine_source &s, int img0, int img1, double x, double y, int *row, int *col) {
    const int H = s.H_ref, W = s.W_ref;
    const double rel0 = (double)H / (double)img0, rel1 = (double)W / (double)img1;
    const double colf = rel0 * x, rowf = rel1 * y;
    if (!(colf > -2147483648.0 && colf < 2147483648.0 && rowf > -2147483648.0 && rowf < 2147483648.0)) return false;
    int c = (int)colf, r = (int)rowf;
    if (r < 0 && r >= -H) r += H;
    if (c < 0 && c >= -W) c += W;
    if (r < 0 || r >= H || c < 0 || c >= W) return false;
    *row = r;
    *col = c;
    return true;
}

// channel c of the map at (row, col), through fp64 (exact for both source dtypes) to the storage dtype
template <typename Tout>
FMPNP_LOC_HD Tout ref_value(const fmpnp_loc_refine_source &s, int c, int row, int col) {
    const size_t at = ((size_t)c * (size_t)s.H_ref + (size_t)row) * (size_t)s.W_ref + (size_t)col;
    const double v = s.dtype == FMPNP_F64 ? ((const double *)s.ref_chw)[at] : (double)((const float *)s.ref_chw)[at];
    return (Tout)v;
}

// host validation shared by the HIP entry points and the twin
inline int refine_args(const fmpnp_loc_query *queries, int n_queries, const fmpnp_loc_refine_map *maps,
                       const fmpnp_loc_refine_params *rp) {
    if (n_queries < 0 || !rp || (n_queries && (!queries || !maps))) return FMPNP_EINVAL;
    if (rp->C < 1 || rp->cstride < rp->C || rp->img0 < 1 || rp->img1 < 1) return FMPNP_EINVAL;
    if (rp->intrinsics != FMPNP_LOC_K_LAST && rp->intrinsics != FMPNP_LOC_K_BEST) return FMPNP_EINVAL;
    if (rp->n_levels < 0 || rp->n_levels > FMPNP_LOC_REFINE_MAX_LEVELS || (rp->n_levels && !rp->levels)) return FMPNP_EINVAL;
    for (int l = 0; l < rp->n_levels; ++l)
        if (rp->levels[l].c_begin < 0 || rp->levels[l].c_end <= rp->levels[l].c_begin || rp->levels[l].c_end > rp->C)
            return FMPNP_EINVAL;
    for (int i = 0; i < n_queries; ++i) {
        if (maps[i].Hf < 1 || maps[i].Wf < 1) return FMPNP_EINVAL;
        if (queries[i].out_offset < 0 || queries[i].out_cap < 0 || queries[i].pair_begin < 0 || queries[i].pair_count < 0)
            return FMPNP_EINVAL;
    }
    return 0;
}

inline RefineLevels refine_levels(const fmpnp_loc_refine_params &rp) {
    RefineLevels lv{};
    lv.n_levels = rp.n_levels;
    for (int l = 0; l < rp.n_levels; ++l) lv.lv[l] = rp.levels[l];
    return lv;
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
