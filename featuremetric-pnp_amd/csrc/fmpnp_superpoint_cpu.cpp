// fmpnp_superpoint_cpu.cpp -- the CPU twins of the SuperPoint baseline's five stages (fmpnp_superpoint.hip)
// with HOST pointers: fmpnp_sp_heatmap_cpu, fmpnp_sp_nms_cpu, fmpnp_sp_describe_cpu, fmpnp_sp_match_cpu and
// fmpnp_sp_assemble_cpu.
//
// Every value comes from fmpnp_superpoint_impl.h, the header the kernels are built from, and this unit is
// compiled without contraction, so every byte the contract names is the GPU's.  The NMS is the greedy walk
// itself (a sort and a grid, as nms_fast has it); the kernels reach the same set in parallel rounds.  The
// scores are the fmaf chain of fmpnp_match_cpu.cpp.  Explicit CPU entry points -- a parity bridge -- never a
// fallback of the HIP entry points.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_superpoint_impl.h"

using namespace fmpnp::sp;

namespace {

constexpr int JB = 1024;  // columns per accumulator block (stays in L1)

}  // namespace

extern "C" {

int fmpnp_sp_heatmap_cpu(const float *semi, int Hc, int Wc, float *heat) {
    const int rc = heat_args(semi, Hc, Wc, heat);
    if (rc) return rc;
    const size_t plane = (size_t)Hc * (size_t)Wc, W = (size_t)Wc * CELL;
    for (int yc = 0; yc < Hc; ++yc)
        for (int xc = 0; xc < Wc; ++xc) {
            const float *cell = semi + (size_t)yc * Wc + xc;
            float *out = heat + (size_t)yc * CELL * W + (size_t)xc * CELL;
            cell_heat([&](int c) { return cell[(size_t)c * plane]; },
                      [&](int c, float v) { out[(size_t)(c / CELL) * W + (size_t)(c % CELL)] = v; });
        }
    return 0;
}

long long fmpnp_sp_nms_capacity(int H, int W, int nms_dist) {
    if (H < 1 || W < 1 || nms_dist < 0 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    return keep_capacity(H, W, nms_dist);
}

int fmpnp_sp_nms_cpu(const float *heat, int H, int W, double conf_thresh, int nms_dist, int border, double *pts,
                     long long ld_pts, int *n) {
    const int rc = nms_args(heat, H, W, conf_thresh, nms_dist, border, pts, ld_pts);
    if (rc) return rc;
    if (!n) return FMPNP_EINVAL;
    const float thresh = (float)conf_thresh;
    const size_t HW = (size_t)H * (size_t)W;
    try {
        std::vector<uint64_t> words;
        for (size_t i = 0; i < HW; ++i)
            if (is_candidate(heat[i], thresh)) words.push_back(nms_word(heat[i], (uint32_t)i));
        std::sort(words.begin(), words.end(), [](uint64_t a, uint64_t b) { return a > b; });
        std::vector<unsigned char> state(HW, EMPTY);
        for (uint64_t w : words) state[fmpnp::rv::word_index(w)] = LIVE;
        int count = 0;
        for (uint64_t w : words) {
            const uint32_t i = fmpnp::rv::word_index(w);
            if (state[i] != LIVE) continue;
            const int x = (int)(i % (uint32_t)W), y = (int)(i / (uint32_t)W);
            for (int v = std::max(0, y - nms_dist); v <= std::min(H - 1, y + nms_dist); ++v)
                for (int u = std::max(0, x - nms_dist); u <= std::min(W - 1, x + nms_dist); ++u)
                    if (state[(size_t)v * W + u] == LIVE) state[(size_t)v * W + u] = GONE;
            state[i] = KEPT;
            if (on_border(x, y, W, H, border)) continue;
            if (count == FMPNP_SP_MAX_KEYPOINTS) return FMPNP_ETOOBIG;
            pts[count] = (double)x;
            pts[ld_pts + count] = (double)y;
            pts[2 * ld_pts + count] = (double)heat[i];
            ++count;
        }
        *n = count;
    } catch (const std::bad_alloc &) {
        return FMPNP_ENOMEM;
    }
    return 0;
}

int fmpnp_sp_describe_cpu(const float *coarse, int D, int Hc, int Wc, const double *pts, long long ld_pts, int N,
                          int H, int W, int align_corners, float *desc, long long ld_desc) {
    const int rc = desc_args(coarse, D, Hc, Wc, pts, ld_pts, N, H, W, align_corners, desc, ld_desc);
    if (rc) return rc;
    const size_t plane = (size_t)Hc * (size_t)Wc;
    for (int p = 0; p < N; ++p) {
        const Taps t = make_taps(pts[p], pts[ld_pts + p], W, H, Wc, Hc, align_corners);
        float chain[CHAINS];
        for (int i = 0; i < CHAINS; ++i) chain[i] = 0.0f;
        for (int c = 0; c < D; ++c) {
            const float v = sample(coarse + (size_t)c * plane, Wc, t);
            desc[(size_t)c * ld_desc + p] = v;
            chain[c % CHAINS] = square_link(v, chain[c % CHAINS]);
        }
        for (int o = CHAINS / 2; o > 0; o >>= 1) {
            float next[CHAINS];
            for (int i = 0; i < CHAINS; ++i) next[i] = chain[i] + chain[i ^ o];
            memcpy(chain, next, sizeof(chain));
        }
        const float norm = desc_norm(chain[0]);
        for (int c = 0; c < D; ++c) desc[(size_t)c * ld_desc + p] = desc[(size_t)c * ld_desc + p] / norm;
    }
    return 0;
}

int fmpnp_sp_match_cpu(const float *desc1, int N1, int ld1, const float *desc2_t, int D, int N2, int ld2, double ratio,
                       int *nn_idx, float *nn_dist, unsigned char *ok, long long *matches, int *count) {
    const int rc = match_args(desc1, N1, ld1, desc2_t, D, N2, ld2, ratio, nn_idx, nn_dist, ok, matches, count);
    if (rc) return rc;
    const float ratio2 = ratio_squared(ratio);
    int n = 0;
    try {
        std::vector<float> row((size_t)N2);
        for (int i = 0; i < N1; ++i) {
            for (int j0 = 0; j0 < N2; j0 += JB)
                fmpnp::host::fmaf_chains(desc1 + (size_t)i * ld1, desc2_t + j0, (size_t)ld2, D, std::min(JB, N2 - j0),
                                         row.data() + j0);
            uint64_t a = NO_WORD, b = NO_WORD;
            for (int j = 0; j < N2; ++j) two_insert(a, b, dist_word(score_dist(row[j]), (uint32_t)j));
            const int j0 = (int)(uint32_t)a, j1 = (int)(uint32_t)b;
            const float d0 = score_dist(row[j0]), d1 = score_dist(row[j1]);
            nn_idx[2 * (size_t)i] = j0;
            nn_idx[2 * (size_t)i + 1] = j1;
            nn_dist[2 * (size_t)i] = d0;
            nn_dist[2 * (size_t)i + 1] = d1;
            ok[i] = ratio_ok(d0, d1, ratio2) ? 1 : 0;
            if (ok[i]) {
                matches[2 * (size_t)n] = i;
                matches[2 * (size_t)n + 1] = j0;
                ++n;
            }
        }
    } catch (const std::bad_alloc &) {
        return FMPNP_ENOMEM;
    }
    *count = n;
    return 0;
}

int fmpnp_sp_assemble_cpu(const double *query_pts, int N1, long long ld_q, const double *ref_pts, int N2,
                          long long ld_r, const double *points2d, const double *points3d, int M,
                          const long long *matches, int n_matches, int *argmin, double *x2d, double *x2d_ref,
                          double *x3d, int *count) {
    const int rc = assemble_args(query_pts, N1, ld_q, ref_pts, N2, ld_r, points2d, points3d, M, matches, n_matches,
                                 argmin, x2d, x2d_ref, x3d, count);
    if (rc) return rc;
    for (int i = 0; i < N2; ++i) {
        const double px = ref_pts[i], py = ref_pts[ld_r + i];
        double best = NO_DIST;
        int best_m = NO_LANDMARK;
        for (int m = 0; m < M; ++m) {
            const double d = landmark_dist(px, py, points2d[2 * (size_t)m], points2d[2 * (size_t)m + 1]);
            if (closer(d, m, best, best_m)) {
                best = d;
                best_m = m;
            }
        }
        argmin[i] = landmark_index(best_m);
    }
    int n = 0;
    try {
        std::vector<int> first((size_t)N2, INT32_MAX);
        for (int m = 0; m < n_matches; ++m) {
            const long long q = matches[2 * (size_t)m], j = matches[2 * (size_t)m + 1];
            if (match_valid(q, j, N1, N2)) first[(size_t)j] = std::min(first[(size_t)j], (int)q);
        }
        for (int i = 0; i < N2; ++i)
            if (first[i] != INT32_MAX)
                write_assembled(query_pts, ld_q, ref_pts, ld_r, points3d, argmin, first[i], i, n++, x2d, x2d_ref, x3d);
    } catch (const std::bad_alloc &) {
        return FMPNP_ENOMEM;
    }
    *count = n;
    return 0;
}

}  // extern "C"
