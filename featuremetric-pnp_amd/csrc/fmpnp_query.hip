// fmpnp_query.hip -- fmpnp_feature_pnp: one query of the reference adapter in ONE host call.
//
// feature_pnp (s2dhm/pose_prediction/optimize_feature_pnp.py:50-71) prepares a query on the
// host -- fref gather, fp64 cast, Sobel -- and then runs forward or multilevel_optimization
// (featurePnP/model.py:178-213, 245-494).  Here the whole call is one stream of device work
// with a single host wait at the end:
//
//   H2D   reference inliers, 3D points and the launch descriptors, one copy from a pinned
//         staging buffer the library owns (no pageable copies, no allocation per call);
//   pack  the query map (fused Sobel + channels-last, or the f-only copy) into a cached buffer;
//   fref  gather of the reference descriptors (out-of-map inliers set a device flag -- the
//         reference's IndexError -- read with the results, no wait here);
//   LM    forward over the whole map, or compute_cost + one forward per channel level, each
//         level's initial pose copied from the previous level's result on the device;
//   D2H   results (+ trace) and the flag, one copy, one stream synchronisation.
//
// The kernels are the ones the separate entry points launch, with the same descriptors, so the
// results equal pack + gather + refine called one by one, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>

#include "fmpnp.h"
#include "fmpnp_hypercolumn_impl.h"
#include "fmpnp_hypercolumn_pack_impl.h"
#include "fmpnp_internal.h"

using namespace fmpnp;

namespace {

std::atomic<long long> g_window_reruns{0};  // fmpnp_feature_pnp calls re-run fully packed after a window miss

}  // namespace

extern "C" int fmpnp_compute_cost_async(const fmpnp_problem *prob, int layout, int dtype, int use_ratio,
                                        double ratio_threshold, double *cost, int *supported, fmpnp_result *result,
                                        void *hip_stream) {
    if (!prob || !result || (prob->N > 0 && (!cost || !supported))) return FMPNP_EINVAL;
    const fmpnp_problem &p = *prob;
    if (layout != FMPNP_LAYOUT_FGRAD && layout != FMPNP_LAYOUT_F) return FMPNP_EINVAL;
    if (dtype != FMPNP_F32 && dtype != FMPNP_F64 && dtype != FMPNP_F16) return FMPNP_EINVAL;
    if (layout == FMPNP_LAYOUT_F && dtype != FMPNP_F32) return FMPNP_EINVAL;
    if (p.N < 0 || p.c_end <= p.c_begin) return FMPNP_EINVAL;
    if (p.N > 0) {
        const int rc = fmpnp_point_costs(prob, layout, dtype, cost, supported, hip_stream);  // (validates the rest)
        if (rc) return rc;
    }
    return (int)launch_cost_mean(p, use_ratio, ratio_threshold, cost, supported, result, (hipStream_t)hip_stream);
}

namespace {

// where the reference descriptors come from: the dense [C][H][W] map (fmpnp_feature_pnp: gathered), or the
// encoder's layers (fmpnp_feature_pnp_layers: the sparse hypercolumn kernel forms the rows, no dense map)
struct RefSource {
    const void *chw;
    int dtype;
    const fmpnp_hc_layer *layers;
    int n_layers, flags;
    int H, W;
};

// where the query map comes from: the dense [C][H][W] map (packed by the Sobel pack), or the encoder's layers
// (fmpnp_feature_pnp_query_layers: the fused hypercolumn pack forms the packed map, no dense map)
struct QuerySource {
    const void *chw;
    int dtype;
    const fmpnp_hc_layer *layers;
    int n_layers, flags;
};

// the body of the entry points; only the pack reads `query` and only the fref step reads `ref`
int feature_pnp_run(const QuerySource &query, int C, int H, int W, const RefSource &ref,
                    const double *ref_inliers, const double *pts3d, int N, const double K[9], const double R0[9],
                    const double t0[3], int img0, int img1, const fmpnp_level *levels, int n_levels,
                    const fmpnp_options *opt, int window_radius, fmpnp_result *results, fmpnp_trace_entry *trace,
                    int trace_stride, void *hip_stream) {
    const int H_ref = ref.H, W_ref = ref.W;
    const void *query_chw = query.chw;
    const int dtype_query = query.dtype;
    if ((!query_chw && !query.layers) || !opt || !results || !K || !R0 || !t0 || N < 0 || C <= 0 || H <= 0 || W <= 0 || H_ref <= 0 ||
        W_ref <= 0 || img0 <= 0 || img1 <= 0 || n_levels < 0 || (n_levels > 0 && !levels))
        return FMPNP_EINVAL;
    if (N > 0 && (!ref_inliers || !pts3d)) return FMPNP_EINVAL;
    if (dtype_query != FMPNP_F32 && dtype_query != FMPNP_F64) return FMPNP_EINVAL;
    if (opt->mode != FMPNP_MODE_FORWARD || (trace && trace_stride < 1)) return FMPNP_EINVAL;
    // packed windows: the fused Sobel pack of the packed f, gx, gy planes, nearest sampling
    if (window_radius < 0 || window_radius > 4096 ||
        (window_radius > 0 && (opt->layout != FMPNP_LAYOUT_FGRAD || opt->sampling != FMPNP_NEAREST)))
        return FMPNP_EINVAL;
    for (int l = 0; l < n_levels; ++l)
        if (levels[l].c_begin < 0 || levels[l].c_end <= levels[l].c_begin || levels[l].c_end > C) return FMPNP_EINVAL;
    const bool lay_f = opt->layout == FMPNP_LAYOUT_F;
    // binary16 storage (include/fmpnp.h): the dense query map and reference map only -- the sparse and fused
    // hypercolumn kernels do not write it; the scratch and the channel stride follow the element size
    const bool f16 = opt->dtype == FMPNP_F16;
    if (f16 && (query.layers || ref.layers)) return FMPNP_EINVAL;
    const int es = opt->dtype == FMPNP_F64 ? 8 : f16 ? 2 : 4;
    const int cs = f16 ? (C + 7) / 8 * 8 : (C + 3) / 4 * 4;
    const int planes = lay_f ? 1 : 3;
    const int n_fwd = n_levels > 0 ? n_levels : 1;
    const int n_res = n_levels > 0 ? n_levels + 1 : 1;  // [compute_cost,] forward per level
    const int stride = trace ? trace_stride : 0;

    // host-side descriptors: [0] compute_cost over the whole map (levels only), then the forwards
    fmpnp_problem hd[1 + 64];
    if (n_res > 65) return FMPNP_EINVAL;
    for (int r = 0; r < n_res; ++r) {
        fmpnp_problem &p = hd[r];
        memset(&p, 0, sizeof(p));
        p.Hf = H;
        p.Wf = W;
        p.cstride = cs;
        p.ld_ref = cs;
        p.N = N;
        p.im_width = img0;
        p.im_height = img1;
        memcpy(p.K, K, sizeof(p.K));
        memcpy(p.R0, R0, sizeof(p.R0));
        memcpy(p.t0, t0, sizeof(p.t0));
        const int l = n_levels > 0 ? r - 1 : 0;
        p.c_begin = (n_levels > 0 && r > 0) ? levels[l].c_begin : 0;
        p.c_end = (n_levels > 0 && r > 0) ? levels[l].c_end : C;
        // (pointers are set below, once the device buffer is placed; the plans need only sizes)
        p.feat = p.fref = (const void *)(uintptr_t)256;
        p.pts3d = (const double *)(uintptr_t)256;
    }
    // the LM workspace of the largest plan (the launches run one after another on the stream)
    // (with and without the window: a window miss re-runs the call fully packed)
    size_t ws = 0;
    for (int wi = 0; wi < (window_radius > 0 ? 2 : 1); ++wi)
        for (int r = n_levels > 0 ? 1 : 0; r < n_res; ++r) {  // (compute_cost: point costs + one reduction)
            fmpnp_problem pw = hd[r];
            pw.window = wi ? (const unsigned char *)(uintptr_t)256 : nullptr;
            const size_t w = fmpnp_workspace_size(&pw, 1, opt);
            if (w == 0) return FMPNP_EINVAL;  // (fmpnp_workspace_size: invalid problem / options)
            ws = std::max(ws, w);
        }
    // device carve: [inl | pts | descs] (the one upload), [results | err | trace] (the one
    // download), the packed map, fref, the LM workspace
    const size_t b_inl = align256((size_t)N * 16), b_pts = align256((size_t)N * 24), b_desc = align256(sizeof(fmpnp_problem) * n_res);
    const size_t b_res = align256(sizeof(fmpnp_result) * n_res), b_err = 256;
    const size_t b_tr = trace ? align256(sizeof(fmpnp_trace_entry) * (size_t)n_fwd * stride) : 0;
    const size_t b_feat = align256((size_t)H * W * planes * cs * es), b_fref = align256((size_t)std::max(N, 1) * cs * es);
    const size_t b_cost = n_levels > 0 ? align256((size_t)std::max(N, 1) * 12) : 0;  // compute_cost's per-point costs
    const size_t up = b_inl + b_pts + b_desc, down = b_res + b_err + b_tr;
    const size_t b_win = window_radius > 0 ? align256((size_t)2 * H * W) : 0;  // [2][H][W] window map
    // a query given as layers: the texels' norms (fmpnp_hypercolumn_pack.hip), formed once per attempt
    const bool q_norm = query.layers && (query.flags & FMPNP_HC_NORMALIZE);
    const size_t b_norm = q_norm ? hc_pack_workspace_bytes(H, W) : 0;
    const size_t need = up + down + b_feat + b_fref + align256(ws) + b_cost + b_win + b_norm;

    hipStream_t s = (hipStream_t)hip_stream;
    // this stream's scratch (fmpnp_internal.h StreamScratch): the device carve and a pinned staging
    // buffer, grown on demand and reused; calls on other streams or devices use their own
    SyncCall call(SCRATCH_QUERY, s, need, up + down, (size_t)64 << 20);
    int rc = call.error();
    if (rc) return rc;
    StreamScratch *sc = call.sc;
    hipError_t e = hipSuccess;
    unsigned char *d = call.dev, *h = call.host;
    double *d_inl = (double *)d, *d_pts = (double *)(d + b_inl);
    fmpnp_problem *d_desc = (fmpnp_problem *)(d + b_inl + b_pts);
    fmpnp_result *d_res = (fmpnp_result *)(d + up);
    int *d_err = (int *)(d + up + b_res);
    fmpnp_trace_entry *d_tr = trace ? (fmpnp_trace_entry *)(d + up + b_res + b_err) : nullptr;
    unsigned char *d_feat = d + up + down, *d_fref = d_feat + b_feat, *d_ws = d_fref + b_fref;
    double *d_cost = (double *)(d_ws + align256(ws));
    int *d_sup = (int *)(d_cost + std::max(N, 1));
    unsigned char *d_win = (unsigned char *)d_cost + b_cost;
    float *d_norm = q_norm ? (float *)(d_win + b_win) : nullptr;
    for (int r = 0; r < n_res; ++r) {
        hd[r].feat = d_feat;
        hd[r].fref = d_fref;
        hd[r].pts3d = d_pts;
    }
    // the first level's channels [sb, se) packed on the main stream and the other channels on the side
    // stream, under the first level's LM launch (one workgroup and its helpers: the rest of the device is
    // idle).  Only with channel boundaries on 128-byte lines (sb, se multiples of 32), so no cache line
    // holds channels of both streams' packs (the split against one pack before the first level:
    // profiles/r06_query_split_ab.txt)
    const int sb = n_levels >= 2 ? levels[0].c_begin : 0, se = n_levels >= 2 ? levels[0].c_end : C;
    const int line = f16 ? 64 : 32;  // (channels per 128 bytes: binary16 holds twice as many)
    const bool split = n_levels >= 2 && !lay_f && (sb > 0 || se < C) && sb % line == 0 &&
                       (se % line == 0 || se == C);
    if (split) {
        const int rc2 = scratch_side(*sc);
        if (rc2) return rc2;
    }
    // Sobel pack of channels [c0, c1) (fmpnp_pack.hip: a channel's gradients read only its own plane, so a
    // channel range is the whole-map pack's bytes for those channels) on stream st
    bool win = false;
    auto pack_range = [&](int c0, int c1, hipStream_t st) -> hipError_t {
        if (query.layers)  // (the f-only layout's padding channels are zeroed beforehand, below)
            return (hipError_t)launch_hc_pack(query.layers, query.n_layers, 0, H, W, C, c0, c1, opt->layout, opt->dtype,
                                              cs, opt->sobel_flags & 1, (opt->sobel_flags >> 1) & 1,
                                              win ? d_win : nullptr, d_norm, d_feat, st);
        const void *src = (const unsigned char *)query_chw + (size_t)c0 * H * W * (dtype_query == FMPNP_F64 ? 8 : 4);
        void *dst = d_feat + (size_t)c0 * es;
        if (win)
            return launch_pack_win(src, dtype_query, c1 - c0, H, W, dst, opt->dtype, cs, opt->sobel_flags & 1,
                                   (opt->sobel_flags >> 1) & 1, d_win, st);
        return launch_pack(src, nullptr, nullptr, dtype_query, c1 - c0, H, W, dst, opt->dtype, cs,
                           opt->sobel_flags & 1, (opt->sobel_flags >> 1) & 1, st, planes);
    };
  for (int attempt = 0; attempt < 2; ++attempt) {
    // attempt 0: windowed when asked; attempt 1 (only after a window miss): the full pack
    win = attempt == 0 && window_radius > 0;
    if (attempt == 1 && window_radius == 0) break;
    for (int r = 0; r < n_res; ++r) hd[r].window = win ? d_win : nullptr;
    // the one upload
    if (N > 0) {
        memcpy(h, ref_inliers, (size_t)N * 16);
        memcpy(h + b_inl, pts3d, (size_t)N * 24);
    }
    memcpy(h + b_inl + b_pts, hd, sizeof(fmpnp_problem) * n_res);
    e = hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(d_err, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (trace) {
        e = hipMemsetAsync(d_tr, 0, b_tr, s);
        if (e != hipSuccess) return (int)e;
    }
    // pack (optimize_feature_pnp.py:57,61): the Sobel pack writes channels < C, so a padded
    // stride is zeroed first; the f-only copy fills the padding itself.  Not for a windowed attempt:
    // its unmarked texels are never trusted anyway (a miss re-runs the call), and no kernel reads a
    // channel >= C (every level's [c_begin, c_end) lies below C), so zeroing the whole map there would
    // only add the full-map write the window exists to avoid
    if ((!lay_f || query.layers) && cs != C && !win) {
        e = hipMemsetAsync(d_feat, 0, b_feat, s);
        if (e != hipSuccess) return (int)e;
    }
    if (win) {
        // only the texels within window_radius of a point's texel at (R0, t0) (its square in plane 0 of
        // the window map): the refinement reads the texels its points visit, a few from where they
        // start; the LM flags a gather outside the window (FMPNP_STATUS_WINDOW) and the call re-runs
        e = launch_win_mark(d_desc, 1, window_radius, N, (long)H * W, s);
        if (e != hipSuccess) return (int)e;
    }
    if (q_norm) {
        // the norms over all C channels, before the first pack; the side stream's packs read them too (it
        // starts after the event below).  A windowed attempt forms them only near the marks, so the fully
        // packed re-run forms them again
        e = (hipError_t)launch_hc_norm(query.layers, query.n_layers, 0, H, W, C, d_norm, win ? d_win : nullptr, s);
        if (e != hipSuccess) return (int)e;
    }
    // with a split, only the first level's channels here; the rest on the side stream below
    e = split ? pack_range(sb, se, s) : pack_range(0, C, s);
    if (e != hipSuccess) return (int)e;
    // fref (optimize_feature_pnp.py:51-56): the reference map's first C channels
    if (N > 0) {
        if (cs != C) {
            e = hipMemsetAsync(d_fref, 0, b_fref, s);
            if (e != hipSuccess) return (int)e;
        }
        if (ref.layers)  // (validated by the entry point: the layers' channels add up to C)
            e = (hipError_t)launch_hypercolumn_sparse(ref.layers, ref.n_layers, 1, H_ref, W_ref, d_inl, nullptr, N,
                                                      FMPNP_HC_AT_REFERENCE, (double)img0, (double)img1, d_fref,
                                                      opt->dtype, cs, C, ref.flags, d_err, s);
        else
            e = launch_gather_ref(ref.chw, ref.dtype, C, H_ref, W_ref, d_inl, N, img0, img1, d_fref, opt->dtype, cs,
                                  d_err, s);
        if (e != hipSuccess) return (int)e;
    }
    if (split) {
        // the side stream: after the first level's pack and the fref gather, the other channels' pack and
        // compute_cost (which reads every channel); the main stream meets it before the second level
        e = hipEventRecord(sc->ev[0], s);
        if (e == hipSuccess) e = hipStreamWaitEvent(sc->side, sc->ev[0], 0);
        if (e == hipSuccess && sb > 0) e = pack_range(0, sb, sc->side);
        if (e == hipSuccess && se < C) e = pack_range(se, C, sc->side);
        if (e != hipSuccess) return (int)e;
        e = launch_compute_cost(hd[0], opt->layout, opt->dtype, opt->use_ratio, opt->ratio_threshold, d_cost, d_sup,
                                d_res, sc->side);
        if (e == hipSuccess) e = hipEventRecord(sc->ev[1], sc->side);
        if (e != hipSuccess) return (int)e;
    }
    // the LM launches
    for (int r = 0; r < n_res; ++r) {
        const bool cost = n_levels > 0 && r == 0;
        if (cost) {
            // compute_cost (model.py:216-243): every point's cost at once (one wave each), one
            // fixed-order reduction -- one evaluation, so not an LM launch (a latency chain there)
            // (with a split it runs on the side stream, above)
            if (!split)
                e = launch_compute_cost(hd[0], opt->layout, opt->dtype, opt->use_ratio, opt->ratio_threshold, d_cost,
                                        d_sup, d_res, s);
            if (e != hipSuccess) return (int)e;
            continue;
        }
        if (split && r == 2) {
            e = hipStreamWaitEvent(s, sc->ev[1], 0);
            if (e != hipSuccess) return (int)e;
        }
        if (n_levels > 0 && r >= 2) {
            // level r - 1 starts from level r - 2's result: R[9], t[3] -> R0[9], t0[3] (contiguous)
            static_assert(offsetof(fmpnp_problem, t0) == offsetof(fmpnp_problem, R0) + 72, "R0, t0 contiguous");
            static_assert(offsetof(fmpnp_result, t) == offsetof(fmpnp_result, R) + 72, "R, t contiguous");
            e = hipMemcpyAsync((unsigned char *)(d_desc + r) + offsetof(fmpnp_problem, R0),
                               (const unsigned char *)(d_res + r - 1) + offsetof(fmpnp_result, R), 96,
                               hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return (int)e;
        }
        fmpnp_trace_entry *tr = (trace && !cost) ? d_tr + (size_t)(n_levels > 0 ? r - 1 : 0) * stride : nullptr;
        rc = fmpnp_refine_batch_async(d_desc + r, &hd[r], 1, N, opt, d_res + r, tr, stride, d_ws, ws, hip_stream);
        if (rc) return rc;
    }
    // the one download
    e = hipMemcpyAsync(h, d_res, down, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    rc = call.finish();  // this attempt's one wait
    if (rc) return rc;
    bool miss = false;
    for (int r = 0; r < n_res; ++r) miss = miss || (((const fmpnp_result *)h)[r].status & FMPNP_STATUS_WINDOW);
    if (win && miss) {
        g_window_reruns.fetch_add(1);
        call.resume();
        continue;  // a point left its window: every result of this attempt is invalid
    }
    memcpy(results, h, sizeof(fmpnp_result) * n_res);
    if (trace) memcpy(trace, h + b_res + b_err, sizeof(fmpnp_trace_entry) * (size_t)n_fwd * stride);
    const int err = *(const int *)(h + b_res);
    return err ? FMPNP_ERANGE : 0;
  }
    return FMPNP_EINVAL;  // (not reached)
}

}  // namespace

extern "C" int fmpnp_feature_pnp(const void *query_chw, int dtype_query, int C, int H, int W, const void *ref_chw,
                                 int dtype_ref, int C_ref, int H_ref, int W_ref, const double *ref_inliers,
                                 const double *pts3d, int N, const double K[9], const double R0[9], const double t0[3],
                                 int img0, int img1, const fmpnp_level *levels, int n_levels,
                                 const fmpnp_options *opt, int window_radius, fmpnp_result *results,
                                 fmpnp_trace_entry *trace, int trace_stride, void *hip_stream) {
    if (!ref_chw || C_ref != C || (dtype_ref != FMPNP_F32 && dtype_ref != FMPNP_F64)) return FMPNP_EINVAL;
    const RefSource ref{ref_chw, dtype_ref, nullptr, 0, 0, H_ref, W_ref};
    const QuerySource query{query_chw, dtype_query, nullptr, 0, 0};
    if (!query_chw) return FMPNP_EINVAL;
    return feature_pnp_run(query, C, H, W, ref, ref_inliers, pts3d, N, K, R0, t0, img0, img1, levels,
                           n_levels, opt, window_radius, results, trace, trace_stride, hip_stream);
}

extern "C" int fmpnp_feature_pnp_layers(const void *query_chw, int dtype_query, int C, int H, int W,
                                        const fmpnp_hc_layer *ref_layers, int n_ref_layers, int H_ref, int W_ref,
                                        int ref_flags, const double *ref_inliers, const double *pts3d, int N,
                                        const double K[9], const double R0[9], const double t0[3], int img0, int img1,
                                        const fmpnp_level *levels, int n_levels, const fmpnp_options *opt,
                                        int window_radius, fmpnp_result *results, fmpnp_trace_entry *trace,
                                        int trace_stride, void *hip_stream) {
    if (ref_flags & ~FMPNP_HC_NORMALIZE) return FMPNP_EINVAL;
    long long C_ref = 0;
    const float probe = 0.0f;  // (the sparse rows have no dense output to check)
    const int rc = hc::check_args(ref_layers, n_ref_layers, 1, &probe, H_ref > 0 ? H_ref : 1, W_ref > 0 ? W_ref : 1, 0, 0,
                                  W_ref > 0 ? W_ref : 1, ref_flags, &C_ref);
    if (rc) return rc;
    if (C_ref != C) return FMPNP_EINVAL;
    const RefSource ref{nullptr, FMPNP_F32, ref_layers, n_ref_layers, ref_flags, H_ref, W_ref};
    const QuerySource query{query_chw, dtype_query, nullptr, 0, 0};
    if (!query_chw) return FMPNP_EINVAL;
    return feature_pnp_run(query, C, H, W, ref, ref_inliers, pts3d, N, K, R0, t0, img0, img1, levels,
                           n_levels, opt, window_radius, results, trace, trace_stride, hip_stream);
}

extern "C" int fmpnp_feature_pnp_query_layers(const fmpnp_hc_layer *query_layers, int n_query_layers, int H, int W,
                                              int query_flags, const void *ref_chw, int dtype_ref,
                                              const fmpnp_hc_layer *ref_layers, int n_ref_layers, int H_ref, int W_ref,
                                              int ref_flags, const double *ref_inliers, const double *pts3d, int N,
                                              const double K[9], const double R0[9], const double t0[3], int img0,
                                              int img1, const fmpnp_level *levels, int n_levels,
                                              const fmpnp_options *opt, int window_radius, fmpnp_result *results,
                                              fmpnp_trace_entry *trace, int trace_stride, void *hip_stream) {
    if ((query_flags | ref_flags) & ~FMPNP_HC_NORMALIZE) return FMPNP_EINVAL;
    if ((ref_chw != nullptr) == (ref_layers != nullptr)) return FMPNP_EINVAL;  // (one reference source)
    const float probe = 0.0f;  // (the packed map and the sparse rows have no dense output to check)
    long long C = 0;
    int rc = hc::check_args(query_layers, n_query_layers, 1, &probe, H, W, 0, 0, W > 0 ? W : 1, query_flags, &C);
    if (rc) return rc;
    if ((long long)H * W >= (1ll << 31)) return FMPNP_ETOOBIG;
    if (ref_layers) {
        long long C_ref = 0;
        rc = hc::check_args(ref_layers, n_ref_layers, 1, &probe, H_ref > 0 ? H_ref : 1, W_ref > 0 ? W_ref : 1, 0, 0,
                            W_ref > 0 ? W_ref : 1, ref_flags, &C_ref);
        if (rc) return rc;
        if (C_ref != C) return FMPNP_EINVAL;
    } else if (dtype_ref != FMPNP_F32 && dtype_ref != FMPNP_F64) {
        return FMPNP_EINVAL;
    }
    const RefSource ref{ref_chw, ref_chw ? dtype_ref : FMPNP_F32, ref_layers, ref_layers ? n_ref_layers : 0, ref_flags,
                        H_ref, W_ref};
    const QuerySource query{nullptr, FMPNP_F32, query_layers, n_query_layers, query_flags};
    return feature_pnp_run(query, (int)C, H, W, ref, ref_inliers, pts3d, N, K, R0, t0, img0, img1, levels, n_levels, opt,
                           window_radius, results, trace, trace_stride, hip_stream);
}

extern "C" long long fmpnp_feature_pnp_reruns(void) { return g_window_reruns.load(); }
