// fmpnp_match_layers.hip -- layered dense matching on gfx950 (include/fmpnp.h, "layered matching"): the match
// stage's scores straight from the query's encoder layers.  The align_corners bilinear resize is linear in the
// layer's values and its weights depend on the texel only, so
//     sum_l sum_c d[off_l + c] * resize(layer_l[c])(p)  =  sum_l resize( sum_c d[off_l + c] * layer_l[c] )(p):
// the correlation runs on each layer at the layer's own resolution and the small score maps are resized and
// summed.  The dense [C][H * W] hypercolumn is never written.
//
//   per layer       corr_kernel of fmpnp_match.hip, one launch: the coarse scores S_l [n][H_l * W_l], the exact-
//                   fp32 fmaf chain over the layer's own channels (ld_sparse picks the descriptor's slice, ld_dense
//                   = the layer's channel stride).
//   norm plane      hc_norm_kernel of fmpnp_hypercolumn_pack.hip (pass 1 of the assembly kernel, 4 bytes per
//                   texel), once per call: every row of every round divides by the same plane.
//   combine_kernel  per (row, texel): the four taps of every coarse map, the bilerps, the ascending sum and the
//                   division, by the functions of fmpnp_match_layers_impl.h that the CPU twin calls too.  Lanes
//                   run along the flat texel index, so a wave's store is one contiguous line of scores[i][.]; a
//                   thread keeps its texel and walks CB_R rows, the layer loop outside the row loop: the taps and
//                   weights are set up once per layer, not per row, and the 4 * CB_R loads of a layer are
//                   independent.  The blocks of one row group are adjacent, so the group's coarse maps (about
//                   100 KB a row at the RobotCar shape) are re-read from L2.
//   select_kernel   of fmpnp_match.hip, unchanged.
// Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fmpnp.h"
#include "fmpnp_internal.h"
#include "fmpnp_match_layers_impl.h"

namespace fmpnp {
namespace {

using namespace ml;

constexpr int CB_NT = 256;  // texels per workgroup
constexpr int CB_R = 8;     // rows per thread
constexpr int CB_MAX_ROWS = 65535 * CB_R;  // (the row groups are the grid's y)

struct CombineArgs {
    const float *coarse[hc::MAX_LAYERS];  // S_l [n][H_l * W_l]
    int Hl[hc::MAX_LAYERS], Wl[hc::MAX_LAYERS];
    const float *norm;                    // [H * W], or NULL: no division
    float *scores;                        // [n][ld_scores]
    size_t ld_scores;
    int L, H, W, n;
};

__global__ __launch_bounds__(CB_NT) void combine_kernel(const CombineArgs a) {
    const int WH = a.H * a.W;
    const long long pl = (long long)blockIdx.x * CB_NT + threadIdx.x;
    if (pl >= WH) return;
    const int p = (int)pl, y = p / a.W, x = p % a.W;
    const int i0 = (int)blockIdx.y * CB_R;  // (uniform: the row guards below do not diverge)
    float t[CB_R];
#pragma unroll
    for (int r = 0; r < CB_R; ++r) t[r] = 0.f;
    for (int l = 0; l < a.L; ++l) {
        const Taps tp = taps_at(a.Hl[l], a.Wl[l], a.H, a.W, y, x);
        const size_t wh = (size_t)a.Hl[l] * (size_t)a.Wl[l];
        const float *m = a.coarse[l] + (size_t)i0 * wh;
        float v[CB_R];
#pragma unroll
        for (int r = 0; r < CB_R; ++r) v[r] = i0 + r < a.n ? resized(m + (size_t)r * wh, tp) : 0.f;
#pragma unroll
        for (int r = 0; r < CB_R; ++r) t[r] = summed(t[r], v[r], l == 0);
    }
    const float n = a.norm ? a.norm[p] : 1.f;
#pragma unroll
    for (int r = 0; r < CB_R; ++r)
        if (i0 + r < a.n) a.scores[(size_t)(i0 + r) * a.ld_scores + (size_t)p] = a.norm ? hc::normalised(t[r], n) : t[r];
}

hipError_t launch_combine(const CombineArgs &a, hipStream_t s) {
    const unsigned tiles = (unsigned)(((long long)a.H * a.W + CB_NT - 1) / CB_NT);
    hipLaunchKernelGGL(combine_kernel, dim3(tiles, (unsigned)((a.n + CB_R - 1) / CB_R)), dim3(CB_NT), 0, s, a);
    return hipGetLastError();
}

// The workspace: [norm plane][the coarse maps of one round, layer by layer][the score rows of one round].  Rows
// per round: what 256 MB of coarse maps and score rows hold (one row at least), as fmpnp_match.hip's rule.
constexpr size_t LAYERS_WS_CAP = (size_t)256 << 20;
inline size_t norm_bytes(int H, int W) { return align256((size_t)H * (size_t)W * sizeof(float)); }
inline size_t row_bytes(long long coarse_floats, int H, int W, bool score_rows) {
    return ((size_t)coarse_floats + (score_rows ? (size_t)H * (size_t)W : 0)) * sizeof(float);
}
inline int round_rows(int N, size_t per_row) {
    const size_t rows = std::max<size_t>(1, LAYERS_WS_CAP / per_row);
    return (int)std::min<size_t>(std::min<size_t>(rows, (size_t)CB_MAX_ROWS), (size_t)std::max(N, 1));
}

// the body of the asynchronous entry points: validated arguments; select: the row reduction behind every round
int run_layers(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L, int item, int H, int W,
               long long coarse_floats, long long C, int flags, bool select, int top_k, double ratio, int *argmax,
               float *top, float *kth, unsigned char *mask, float *scores, void *workspace, size_t workspace_bytes,
               hipStream_t s) {
    const size_t b_norm = norm_bytes(H, W), per_row = row_bytes(coarse_floats, H, W, !scores);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < b_norm + per_row) return FMPNP_EINVAL;
    // a round's rows: the rule's, or as many as the caller's workspace holds (a row's bits do not depend on it)
    const int chunk = (int)std::min<size_t>((size_t)round_rows(N, per_row), (workspace_bytes - b_norm) / per_row);
    const int WH = H * W;
    float *norm = nullptr;
    if (flags & FMPNP_HC_NORMALIZE) {
        norm = (float *)workspace;
        const int e = launch_hc_norm(layers, L, item, H, W, C, norm, nullptr, s);
        if (e) return e;
    }
    float *coarse0 = (float *)((unsigned char *)workspace + b_norm);
    float *rows_ws = coarse0 + (size_t)coarse_floats * (size_t)chunk;
    const float ratio2 = (float)(ratio * ratio);
    for (int i0 = 0; i0 < N; i0 += chunk) {  // (stream order: a round's readers run before the next round writes)
        const int n = std::min(chunk, N - i0);
        CombineArgs a = {};
        float *cl = coarse0;
        int off = 0;
        for (int l = 0; l < L; ++l) {
            const fmpnp_hc_layer &ly = layers[l];
            const int wh = ly.H * ly.W;
            const hipError_t e = launch_corr(sparse + (size_t)i0 * (size_t)ld_sparse + off, n, ld_sparse,
                                             ly.data + (size_t)item * (size_t)ly.stride_b, ly.C, wh, (int)ly.stride_c, cl,
                                             (size_t)wh, s);
            if (e != hipSuccess) return (int)e;
            a.coarse[l] = cl;
            a.Hl[l] = ly.H;
            a.Wl[l] = ly.W;
            cl += (size_t)wh * (size_t)chunk;
            off += ly.C;
        }
        float *dst = scores ? scores + (size_t)i0 * (size_t)WH : rows_ws;
        a.norm = norm;
        a.scores = dst;
        a.ld_scores = (size_t)WH;
        a.L = L;
        a.H = H;
        a.W = W;
        a.n = n;
        hipError_t e = launch_combine(a, s);
        if (e != hipSuccess) return (int)e;
        if (select) {
            e = launch_select(dst, (size_t)WH, n, WH, top_k, ratio2, argmax + i0, top + i0, kth + i0, mask + i0, s);
            if (e != hipSuccess) return (int)e;
        }
    }
    return 0;
}

}  // namespace
}  // namespace fmpnp

using namespace fmpnp;

extern "C" {

size_t fmpnp_match_layers_workspace_size(const fmpnp_hc_layer *layers, int L, int N, int H, int W) {
    if (N <= 0 || H < 1 || W < 1 || L < 1 || L > hc::MAX_LAYERS || !layers) return 0;
    long long coarse = 0;
    for (int l = 0; l < L; ++l) {
        if (layers[l].H < 1 || layers[l].W < 1) return 0;
        coarse += (long long)layers[l].H * layers[l].W;
    }
    if (H > hc::MAX_SIZE || W > hc::MAX_SIZE || coarse > (long long)hc::MAX_LAYERS * ml::MAX_WH) return 0;
    const size_t per_row = row_bytes(coarse, H, W, true);
    return norm_bytes(H, W) + (size_t)round_rows(N, per_row) * per_row;
}

int fmpnp_exhaustive_match_layers_async(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L,
                                        int B, int item, int H, int W, int flags, int top_k, double ratio, int *argmax,
                                        float *top, float *kth, unsigned char *mask, float *scores, void *workspace,
                                        size_t workspace_bytes, void *hip_stream) {
    long long C = 0, coarse = 0;
    const int rc = ml::check_args(sparse, N, ld_sparse, layers, L, B, item, H, W, flags, &C, &coarse);
    if (rc) return rc;
    if (top_k < 1 || top_k > H * W || !(ratio == ratio)) return FMPNP_EINVAL;
    if (N == 0) return 0;
    if (!argmax || !top || !kth || !mask) return FMPNP_EINVAL;
    return run_layers(sparse, N, ld_sparse, layers, L, item, H, W, coarse, C, flags, true, top_k, ratio, argmax, top, kth,
                      mask, scores, workspace, workspace_bytes, (hipStream_t)hip_stream);
}

int fmpnp_correlation_layers_async(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L, int B,
                                   int item, int H, int W, int flags, float *scores, void *workspace,
                                   size_t workspace_bytes, void *hip_stream) {
    long long C = 0, coarse = 0;
    const int rc = ml::check_args(sparse, N, ld_sparse, layers, L, B, item, H, W, flags, &C, &coarse);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!scores) return FMPNP_EINVAL;
    return run_layers(sparse, N, ld_sparse, layers, L, item, H, W, coarse, C, flags, false, 1, 0.0, nullptr, nullptr,
                      nullptr, nullptr, scores, workspace, workspace_bytes, (hipStream_t)hip_stream);
}

// the synchronous call: one carve of the (device, stream)'s scratch, one run and one download
int fmpnp_exhaustive_match_layers(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers, int L, int B,
                                  int item, int H, int W, int flags, int top_k, double ratio, int *argmax, float *top,
                                  float *kth, unsigned char *mask, float *scores_dev, void *hip_stream) {
    long long C = 0, coarse = 0;
    const int rc0 = ml::check_args(sparse, N, ld_sparse, layers, L, B, item, H, W, flags, &C, &coarse);
    if (rc0) return rc0;
    if (top_k < 1 || top_k > H * W || !(ratio == ratio)) return FMPNP_EINVAL;
    if (N == 0) return 0;
    if (!argmax || !top || !kth || !mask) return FMPNP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    // the caller's scores_dev takes the score rows' place
    const size_t per_row = row_bytes(coarse, H, W, !scores_dev);
    const size_t b_ws = align256(norm_bytes(H, W) + (size_t)round_rows(N, per_row) * per_row);
    const size_t b_i = align256(sizeof(int) * (size_t)N), b_f = align256(sizeof(float) * (size_t)N), b_m = align256((size_t)N);
    SyncCall call(SCRATCH_MATCH, s, b_ws + b_i + 2 * b_f + b_m, 0);
    if (call.error()) return call.error();
    unsigned char *base = call.dev;
    int *d_arg = (int *)(base + b_ws);
    float *d_top = (float *)(base + b_ws + b_i), *d_kth = (float *)(base + b_ws + b_i + b_f);
    unsigned char *d_mask = base + b_ws + b_i + 2 * b_f;
    const int rc = run_layers(sparse, N, ld_sparse, layers, L, item, H, W, coarse, C, flags, true, top_k, ratio, d_arg,
                              d_top, d_kth, d_mask, scores_dev, base, b_ws, s);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(argmax, d_arg, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(top, d_top, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(kth, d_kth, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(mask, d_mask, (size_t)N, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    return call.finish();
}

}  // extern "C"
