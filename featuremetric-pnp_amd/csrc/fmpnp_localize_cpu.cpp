// fmpnp_localize_cpu.cpp -- fmpnp_localize_build_cpu and fmpnp_localize_pick_cpu: the CPU twins of the
// localisation chain's two glue kernels (fmpnp_localize.hip) with HOST pointers; and
// fmpnp_localize_refine_prep_cpu, the twin of the refinement stage's prep and gather kernels
// (fmpnp_localize_refine.hip).
//
// Every value comes from fmpnp_localize_impl.h, the header the kernels are built from, and this unit is
// compiled without contraction, so every byte the contract names is the GPU's.  A row's place in the
// compacted list is a plain counter here (the kernels find the same place by ballot and running base).
// Explicit CPU entry points -- a parity bridge -- never a fallback of the HIP entry point.
#include "fmpnp.h"
#include "fmpnp_localize_impl.h"

using namespace fmpnp::loc;

extern "C" {

int fmpnp_localize_build_cpu(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_params *params,
                             const int *argmax, const unsigned char *mask, long long total_rows,
                             const fmpnp_loc_matches *matches, fmpnp_pnp_problem *probs) {
    const int rc = pairs_args(pairs, n_pairs, params, total_rows);
    if (rc) return rc;
    if (loc_null(matches)) return FMPNP_EINVAL;
    if (n_pairs && !probs) return FMPNP_EINVAL;
    if (n_pairs && total_rows && (!argmax || !mask)) return FMPNP_EINVAL;
    for (int b = 0; b < n_pairs; ++b) {
        const fmpnp_loc_pair &p = pairs[b];
        int count = 0;
        for (int i = 0; i < p.n_rows; ++i)
            if (mask[(size_t)p.row_offset + (size_t)i] != 0) write_match(p, argmax, *matches, i, count++);
        matches->counts[b] = count;
        write_problem(p, *params, *matches, count, probs[b]);
    }
    return 0;
}

int fmpnp_localize_pick_cpu(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_query *queries, int n_queries,
                            const fmpnp_loc_params *params, const fmpnp_pnp_result *results,
                            const unsigned char *pnp_mask, long long total_rows, const fmpnp_loc_matches *matches,
                            const fmpnp_loc_best *best) {
    int rc = pairs_args(pairs, n_pairs, params, total_rows);
    if (rc) return rc;
    rc = queries_args(pairs, n_pairs, queries, n_queries, total_rows);
    if (rc) return rc;
    if (loc_null(matches) || loc_null(best)) return FMPNP_EINVAL;
    if (n_pairs && (!results || (total_rows && !pnp_mask))) return FMPNP_EINVAL;
    for (int b = 0; b < n_queries; ++b) {
        const fmpnp_loc_query &q = queries[b];
        int kind;
        const int j = pick_best(pairs, q, *params, results, &kind);
        write_record(pairs, q, *params, results, matches->counts, j, kind, best->records[b]);
        if (j < 0) continue;
        const fmpnp_loc_pair &p = pairs[q.pair_begin + j];
        const int count = matches->counts[q.pair_begin + j];
        if (kind == FMPNP_LOC_FALLBACK) {
            for (int m = 0; m < count; ++m) write_best_row(p, q, *matches, *best, m, m);
            continue;
        }
        const bool masked = params->return_masked != 0;
        int n_in = 0;
        for (int m = 0; m < count; ++m) {
            const bool keep = pnp_mask[(size_t)p.row_offset + (size_t)m] != 0;
            if (keep) best->idx[(size_t)q.out_offset + (size_t)n_in] = m;
            if (masked) {
                if (keep) write_best_row(p, q, *matches, *best, m, n_in);
            } else {
                write_best_row(p, q, *matches, *best, m, m);
            }
            n_in += keep ? 1 : 0;
        }
    }
    return 0;
}

}  // extern "C"

namespace {

// the rows of one query, as loc_refine_gather_kernel writes them
template <typename Tout>
void refine_rows(const fmpnp_loc_query &q, const fmpnp_loc_refine_source &s, const fmpnp_loc_refine_params &rp,
                 const fmpnp_loc_best &best, int N, Tout *fref, int *flag) {
    for (int n = 0; n < N; ++n) {
        const size_t t = (size_t)q.out_offset + (size_t)n;
        Tout *row_out = fref + t * (size_t)rp.cstride;
        int row = 0, col = 0;
        const bool ok = ref_cell(s, rp.img0, rp.img1, best.ref2d[2 * t], best.ref2d[2 * t + 1], &row, &col);
        if (!ok) *flag |= 1;
        for (int c = 0; c < rp.cstride; ++c) row_out[c] = (ok && c < rp.C) ? ref_value<Tout>(s, c, row, col) : (Tout)0;
    }
}

}  // namespace

extern "C" int fmpnp_localize_refine_prep_cpu(const fmpnp_loc_pair *pairs, int n_pairs, const fmpnp_loc_query *queries,
                                              int n_queries, const fmpnp_loc_refine_source *sources,
                                              const fmpnp_loc_refine_map *maps, const fmpnp_loc_refine_params *params,
                                              int dtype, const fmpnp_loc_best *best, fmpnp_problem *probs, void *fref,
                                              int *flags) {
    const int rc = refine_args(queries, n_queries, maps, params);
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs && (!pairs || !sources)) || loc_null(best)) return FMPNP_EINVAL;
    if (dtype != FMPNP_F32 && dtype != FMPNP_F64) return FMPNP_EINVAL;
    if (n_queries && (!probs || !fref || !flags)) return FMPNP_EINVAL;
    for (int b = 0; b < n_queries; ++b)
        if ((long long)queries[b].pair_begin + queries[b].pair_count > n_pairs) return FMPNP_EINVAL;
    for (int g = 0; g < n_pairs; ++g)
        if (sources[g].ref_chw && (sources[g].H_ref < 1 || sources[g].W_ref < 1 ||
                                   (sources[g].dtype != FMPNP_F32 && sources[g].dtype != FMPNP_F64)))
            return FMPNP_EINVAL;
    const RefineLevels lv = refine_levels(*params);
    const int n_res = refine_n_res(params->n_levels), es = dtype == FMPNP_F64 ? 8 : 4;
    for (int b = 0; b < n_queries; ++b) {
        const fmpnp_loc_query &q = queries[b];
        const fmpnp_loc_record &rec = best->records[b];
        for (int r = 0; r < n_res; ++r)
            write_refine_problem(pairs, q, rec, sources, maps[b], *params, lv, *best, fref, es, r,
                                 probs[(size_t)r * n_queries + b]);
        flags[b] = 0;
        const int g = refine_pair(q, rec, sources);
        if (g < 0) continue;
        const int N = refine_count(q, rec, sources);
        if (dtype == FMPNP_F64) refine_rows<double>(q, sources[g], *params, *best, N, (double *)fref, &flags[b]);
        else refine_rows<float>(q, sources[g], *params, *best, N, (float *)fref, &flags[b]);
    }
    return 0;
}
