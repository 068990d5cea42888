// fmpnp_localize_cpu.cpp -- fmpnp_localize_build_cpu and fmpnp_localize_pick_cpu: the CPU twins of the
// localisation chain's two glue kernels (fmpnp_localize.hip) with HOST pointers.
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
