// fmpnp_superpoint.hip -- the SuperPoint baseline between the network's two output tensors and the 2D-3D
// matches on gfx950 (include/fmpnp.h, "SuperPoint baseline"; demo_superpoint.py:151-284,
// keypoint_association.py:77-108, superpoint_predictor.py:45-65).
//
//   sp_heat_kernel        one lane per detector cell: 65 exponentials, their ordered sum, 64 heat values.
//   nms_init_kernel       the candidates (heat >= threshold) become live in a byte map of the image.
//   nms_round_kernel<0>   a live candidate with a kept point in its window becomes suppressed.
//   nms_round_kernel<1>   a live candidate whose order word beats every live or newly kept candidate of its
//                         window becomes kept; the candidates still live are counted.  A pixel's byte is
//                         written by its own lane only and the two steps are two launches, so no lane waits
//                         on another workgroup.  Both scan their windows in an LDS tile with a halo; a tile
//                         without a live candidate leaves before loading it.  The host queues `group` rounds
//                         and reads the counts back through pinned memory.  Every round settles at least the
//                         greatest live candidate.
//   nms_count_kernel / nms_compact_kernel   the kept interior points in row-major order: per-chunk counts,
//                         then ballot + popcount + running base behind the sum of the earlier chunks' counts.
//   nms_sort_kernel       the descending order: each point's rank is the number of greater order words,
//                         counted through LDS tiles (the words are distinct, so the ranks are a permutation).
//   sp_desc_kernel        one wave per keypoint, lanes along the channels: four taps, 64 chains of squares,
//                         a butterfly, one division per channel.
//   nn2_kernel            one workgroup per score row: the two smallest distance words per lane, merged
//                         through the wave and LDS; the ratio test.
//   compact_matches_kernel, closest_kernel, first_match_kernel, assemble_kernel   the match list, the nearest
//                         landmark per reference keypoint, the lowest query row per reference keypoint (an
//                         integer atomicMin: order-free) and the assembled arrays, compacted in order.
//
// Every value is formed by fmpnp_superpoint_impl.h, which the CPU twins share.
#include <string.h>

#include <algorithm>

#include "fmpnp_internal.h"
#include "fmpnp_superpoint_impl.h"

namespace fmpnp {
namespace {

using namespace sp;

constexpr int SP_NT = 256;
constexpr int SP_WAVES = SP_NT / 64;

// the place of this lane's kept item among the tile's kept items, and the tile's total (every lane calls it)
__device__ __forceinline__ int tile_place(bool keep, int *wsum, int *total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long b = __ballot(keep);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int before = 0, sum = 0;
    for (int k = 0; k < SP_WAVES; ++k) {
        const int c = wsum[k];
        before += k < w ? c : 0;
        sum += c;
    }
    __syncthreads();  // (the next tile overwrites wsum)
    *total = sum;
    return before + pre;
}

// ---- 1. detector head -------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_NT) void sp_heat_kernel(const float *__restrict__ semi, int Hc, int Wc,
                                                     float *__restrict__ heat) {
    const size_t plane = (size_t)Hc * (size_t)Wc, cell_id = (size_t)blockIdx.x * SP_NT + threadIdx.x;
    if (cell_id >= plane) return;
    const int yc = (int)(cell_id / (size_t)Wc), xc = (int)(cell_id % (size_t)Wc);
    const size_t W = (size_t)Wc * CELL;
    const float *cell = semi + cell_id;
    float *out = heat + (size_t)yc * CELL * W + (size_t)xc * CELL;
    cell_heat([&](int c) { return cell[(size_t)c * plane]; },
              [&](int c, float v) { out[(size_t)(c / CELL) * W + (size_t)(c % CELL)] = v; });
}

// ---- 2. NMS -----------------------------------------------------------------------------------------------
constexpr int TX = 32, TY = 8;  // a tile's interior: one pixel per lane
constexpr int TILE_MAX = (TX + 2 * MAX_DIST) * (TY + 2 * MAX_DIST);
constexpr int CHUNK = 4096;     // pixels per workgroup of the compaction
constexpr int MAX_GROUP = 64;
constexpr int CNT_CAND = 0, CNT_KEPT = 1, CNT_LIVE = 2, N_COUNTERS = CNT_LIVE + MAX_GROUP;

__global__ __launch_bounds__(SP_NT) void nms_init_kernel(const float *__restrict__ heat, size_t HW, float thresh,
                                                      unsigned char *__restrict__ state, int *__restrict__ counters) {
    const size_t i = (size_t)blockIdx.x * SP_NT + threadIdx.x;
    const bool cand = i < HW && is_candidate(heat[i], thresh);
    if (i < HW) state[i] = cand ? LIVE : EMPTY;
    const unsigned long long b = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counters[CNT_CAND], __popcll(b));
}

template <int KEEP>
__global__ __launch_bounds__(SP_NT) void nms_round_kernel(const float *__restrict__ heat, int H, int W, int d,
                                                       unsigned char *__restrict__ state, int *__restrict__ live) {
    __shared__ unsigned char st[TILE_MAX];
    __shared__ float ht[KEEP ? TILE_MAX : 1];
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, x = x0 + tx, y = y0 + ty;
    const bool inside = x < W && y < H;
    const size_t me = (size_t)y * (size_t)W + (size_t)x;
    const bool alive = inside && state[me] == LIVE;
    if (!__syncthreads_or(alive)) return;  // (uniform: no live candidate in this tile)
    const int tw = TX + 2 * d, th = TY + 2 * d;
    for (int e = tid; e < tw * th; e += SP_NT) {
        const int gx = x0 - d + e % tw, gy = y0 - d + e / tw;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t g = (size_t)gy * (size_t)W + (size_t)gx;
        st[e] = in ? state[g] : (unsigned char)EMPTY;
        if (KEEP) ht[e] = in ? heat[g] : 0.0f;
    }
    __syncthreads();
    bool still = false;
    if (alive) {
        const int cx = tx + d, cy = ty + d;  // this lane's place in the tile
        if (!KEEP) {
            bool hit = false;
            for (int v = cy - d; v <= cy + d; ++v)
                for (int u = cx - d; u <= cx + d; ++u) hit |= st[v * tw + u] == KEPT;
            if (hit) state[me] = GONE;
        } else {
            // (after the suppress step no earlier kept point is in a live candidate's window: a kept byte seen
            // here is a neighbour kept by this launch, which beats this candidate as it did while live)
            const uint64_t mine = nms_word(ht[cy * tw + cx], (uint32_t)me);
            bool beaten = false;
            for (int v = cy - d; v <= cy + d; ++v)
                for (int u = cx - d; u <= cx + d; ++u) {
                    const unsigned char s = st[v * tw + u];
                    const int gx = x0 - d + u, gy = y0 - d + v;
                    const uint64_t w = nms_word(ht[v * tw + u], (uint32_t)((size_t)gy * (size_t)W + (size_t)gx));
                    beaten |= (s == LIVE || s == KEPT) && w > mine;
                }
            if (!beaten) state[me] = KEPT;
            still = beaten;
        }
    }
    if (KEEP) {
        const unsigned long long b = __ballot(still);
        if ((tid & 63) == 0 && b) atomicAdd(live, __popcll(b));
    }
}

__device__ __forceinline__ bool kept_inside(const unsigned char *state, size_t i, size_t HW, int W, int H, int border) {
    if (i >= HW || state[i] != KEPT) return false;
    return !on_border((int)(i % (size_t)W), (int)(i / (size_t)W), W, H, border);
}

__global__ __launch_bounds__(SP_NT) void nms_count_kernel(const unsigned char *__restrict__ state, size_t HW, int W, int H,
                                                       int border, int *__restrict__ chunk_count) {
    __shared__ int wsum[SP_WAVES];
    const size_t c0 = (size_t)blockIdx.x * CHUNK;
    int n = 0;
    for (int t = 0; t < CHUNK; t += SP_NT) n += kept_inside(state, c0 + t + threadIdx.x, HW, W, H, border) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < SP_WAVES; ++k) s += wsum[k];
        chunk_count[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(SP_NT) void nms_compact_kernel(const unsigned char *__restrict__ state,
                                                         const float *__restrict__ heat, size_t HW, int W, int H,
                                                         int border, const int *__restrict__ chunk_count,
                                                         uint64_t *__restrict__ words, long long cap,
                                                         int *__restrict__ counters, int *__restrict__ count_out) {
    __shared__ int wsum[SP_WAVES];
    __shared__ int s_base;
    int n = 0;  // the kept points of the earlier chunks
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += SP_NT) n += chunk_count[b];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < SP_WAVES; ++k) s += wsum[k];
        s_base = s;
    }
    __syncthreads();
    int base = s_base;
    const size_t c0 = (size_t)blockIdx.x * CHUNK;
    for (int t = 0; t < CHUNK; t += SP_NT) {  // (uniform trip count: the barriers inside are safe)
        const size_t i = c0 + t + threadIdx.x;
        const bool keep = kept_inside(state, i, HW, W, H, border);
        int total;
        const int place = tile_place(keep, wsum, &total);
        if (keep && (long long)(base + place) < cap) words[base + place] = nms_word(heat[i], (uint32_t)i);
        base += total;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        counters[CNT_KEPT] = base;
        if (count_out) *count_out = base;
    }
}

__global__ __launch_bounds__(SP_NT) void nms_sort_kernel(const uint64_t *__restrict__ words, int n,
                                                      const float *__restrict__ heat, int W, double *__restrict__ pts,
                                                      long long ld_pts) {
    __shared__ uint64_t tile[SP_NT];
    const int i = blockIdx.x * SP_NT + threadIdx.x;
    const uint64_t mine = i < n ? words[i] : 0;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += SP_NT) {  // (uniform trip count)
        tile[threadIdx.x] = t0 + (int)threadIdx.x < n ? words[t0 + threadIdx.x] : 0;
        __syncthreads();
        const int m = min(SP_NT, n - t0);
        for (int j = 0; j < m; ++j) rank += tile[j] > mine ? 1 : 0;
        __syncthreads();
    }
    if (i < n) {  // (distinct words: rank < n <= ld_pts)
        const uint32_t pixel = rv::word_index(mine);
        pts[rank] = (double)(pixel % (uint32_t)W);
        pts[ld_pts + rank] = (double)(pixel / (uint32_t)W);
        pts[2 * ld_pts + rank] = (double)heat[pixel];
    }
}

// ---- 3. descriptors ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_NT) void sp_desc_kernel(const float *__restrict__ coarse, int D, int Hc, int Wc,
                                                     const double *__restrict__ pts, long long ld_pts, int N, int H,
                                                     int W, int align_corners, float *__restrict__ desc,
                                                     long long ld_desc) {
    const int p = blockIdx.x * SP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= N) return;  // (uniform per wave)
    const Taps t = make_taps(pts[p], pts[ld_pts + p], W, H, Wc, Hc, align_corners);
    const size_t plane = (size_t)Hc * (size_t)Wc;
    float chain = 0.0f;
    for (int c = lane; c < D; c += CHAINS) {
        const float v = sample(coarse + (size_t)c * plane, Wc, t);
        desc[(size_t)c * (size_t)ld_desc + (size_t)p] = v;
        chain = square_link(v, chain);
    }
    for (int o = CHAINS / 2; o > 0; o >>= 1) chain = chain + __shfl_xor(chain, o, 64);
    const float norm = desc_norm(chain);
    for (int c = lane; c < D; c += CHAINS) {  // (each lane reads back what it wrote)
        float *q = desc + (size_t)c * (size_t)ld_desc + (size_t)p;
        *q = *q / norm;
    }
}

// ---- 4. two nearest neighbours ----------------------------------------------------------------------------
__global__ __launch_bounds__(SP_NT) void nn2_kernel(const float *__restrict__ scores, size_t ld_scores, int N2, float ratio2,
                                                 int *__restrict__ nn_idx, float *__restrict__ nn_dist,
                                                 unsigned char *__restrict__ ok) {
    __shared__ uint64_t wa[SP_WAVES], wb[SP_WAVES];
    const float *row = scores + (size_t)blockIdx.x * ld_scores;
    uint64_t a = NO_WORD, b = NO_WORD;
    for (int j = threadIdx.x; j < N2; j += SP_NT) two_insert(a, b, dist_word(score_dist(row[j]), (uint32_t)j));
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64);
        two_insert(a, b, oa);
        two_insert(a, b, ob);
    }
    if ((threadIdx.x & 63) == 0) {
        wa[threadIdx.x >> 6] = a;
        wb[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SP_WAVES; ++k) {
            two_insert(a, b, wa[k]);
            two_insert(a, b, wb[k]);
        }
        const int j0 = (int)(uint32_t)a, j1 = (int)(uint32_t)b;  // (N2 >= 2: both are columns of the row)
        const float d0 = score_dist(row[j0]), d1 = score_dist(row[j1]);
        const size_t i = blockIdx.x;
        nn_idx[2 * i] = j0;
        nn_idx[2 * i + 1] = j1;
        nn_dist[2 * i] = d0;
        nn_dist[2 * i + 1] = d1;
        ok[i] = ratio_ok(d0, d1, ratio2) ? 1 : 0;
    }
}

__global__ __launch_bounds__(SP_NT) void compact_matches_kernel(const unsigned char *__restrict__ ok,
                                                             const int *__restrict__ nn_idx, int N1,
                                                             long long *__restrict__ matches, int *__restrict__ count) {
    __shared__ int wsum[SP_WAVES];
    int base = 0;
    for (int t0 = 0; t0 < N1; t0 += SP_NT) {  // (uniform trip count)
        const int i = t0 + threadIdx.x;
        const bool keep = i < N1 && ok[i] != 0;
        int total;
        const int place = tile_place(keep, wsum, &total);
        if (keep) {
            matches[2 * (size_t)(base + place)] = i;
            matches[2 * (size_t)(base + place) + 1] = nn_idx[2 * (size_t)i];
        }
        base += total;
    }
    if (threadIdx.x == 0) *count = base;
}

// ---- 5. association and assembly --------------------------------------------------------------------------
__global__ __launch_bounds__(SP_NT) void closest_kernel(const double *__restrict__ ref_pts, int N2, long long ld_r,
                                                     const double *__restrict__ points2d, int M,
                                                     int *__restrict__ argmin, int *__restrict__ first) {
    const int i = blockIdx.x * SP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N2) return;  // (uniform per wave)
    const double px = ref_pts[i], py = ref_pts[ld_r + i];
    double best = NO_DIST;
    int best_m = NO_LANDMARK;
    for (int m = lane; m < M; m += 64) {
        const double dd = landmark_dist(px, py, points2d[2 * (size_t)m], points2d[2 * (size_t)m + 1]);
        if (closer(dd, m, best, best_m)) {
            best = dd;
            best_m = m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(best, o, 64);
        const int om = __shfl_xor(best_m, o, 64);
        if (closer(od, om, best, best_m)) {
            best = od;
            best_m = om;
        }
    }
    if (lane == 0) {
        argmin[i] = landmark_index(best_m);
        first[i] = INT32_MAX;
    }
}

__global__ __launch_bounds__(SP_NT) void first_match_kernel(const long long *__restrict__ matches, int n, int N1, int N2,
                                                         int *__restrict__ first) {
    const int m = blockIdx.x * SP_NT + threadIdx.x;
    if (m >= n) return;
    const long long q = matches[2 * (size_t)m], j = matches[2 * (size_t)m + 1];
    if (match_valid(q, j, N1, N2)) atomicMin(&first[j], (int)q);
}

__global__ __launch_bounds__(SP_NT) void assemble_kernel(const double *__restrict__ query_pts, long long ld_q,
                                                      const double *__restrict__ ref_pts, int N2, long long ld_r,
                                                      const double *__restrict__ points3d,
                                                      const int *__restrict__ argmin, const int *__restrict__ first,
                                                      double *__restrict__ x2d, double *__restrict__ x2d_ref,
                                                      double *__restrict__ x3d, int *__restrict__ count) {
    __shared__ int wsum[SP_WAVES];
    int base = 0;
    for (int t0 = 0; t0 < N2; t0 += SP_NT) {  // (uniform trip count)
        const int i = t0 + threadIdx.x;
        const int q = i < N2 ? first[i] : INT32_MAX;
        const bool keep = q != INT32_MAX;
        int total;
        const int place = tile_place(keep, wsum, &total);
        if (keep) write_assembled(query_pts, ld_q, ref_pts, ld_r, points3d, argmin, q, i, base + place, x2d, x2d_ref, x3d);
        base += total;
    }
    if (threadIdx.x == 0) *count = base;
}

struct NmsLayout {
    size_t o_words, o_state, o_chunks, o_counters, bytes;
    int n_chunks;
    long long cap;
};
inline NmsLayout nms_layout(int H, int W, int d) {
    NmsLayout l;
    const size_t HW = (size_t)H * (size_t)W;
    l.cap = keep_capacity(H, W, d);
    l.n_chunks = (int)((HW + CHUNK - 1) / CHUNK);
    l.o_words = 0;
    l.o_state = align256(8 * (size_t)l.cap);
    l.o_chunks = l.o_state + align256(HW);
    l.o_counters = l.o_chunks + align256(4 * (size_t)l.n_chunks);
    l.bytes = l.o_counters + align256(4 * N_COUNTERS);
    return l;
}

}  // namespace
}  // namespace fmpnp

using namespace fmpnp;

extern "C" {

int fmpnp_sp_heatmap_async(const float *semi, int Hc, int Wc, float *heat, void *hip_stream) {
    const int rc = heat_args(semi, Hc, Wc, heat);
    if (rc) return rc;
    const size_t cells = (size_t)Hc * (size_t)Wc;
    if (!cells) return 0;
    hipLaunchKernelGGL(sp_heat_kernel, dim3((unsigned)((cells + SP_NT - 1) / SP_NT)), dim3(SP_NT), 0, (hipStream_t)hip_stream, semi,
                       Hc, Wc, heat);
    return (int)hipGetLastError();
}

int fmpnp_sp_heatmap(const float *semi, int Hc, int Wc, float *heat_host, void *hip_stream) {
    const int rc0 = heat_args(semi, Hc, Wc, heat_host);
    if (rc0) return rc0;
    const size_t bytes = 4 * (size_t)Hc * (size_t)Wc * DUST;
    if (!bytes) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    SyncCall call(SCRATCH_SUPERPOINT, s, bytes, 0);
    if (call.error()) return call.error();
    const int rc = fmpnp_sp_heatmap_async(semi, Hc, Wc, (float *)call.dev, hip_stream);
    if (rc) return rc;
    const hipError_t e = hipMemcpyAsync(heat_host, call.dev, bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    return call.finish();
}

size_t fmpnp_sp_nms_workspace_size(int H, int W, int nms_dist) {
    if (H < 1 || W < 1 || nms_dist < 0 || H > MAX_SIDE || W > MAX_SIDE || nms_dist > MAX_DIST) return 0;
    return nms_layout(H, W, nms_dist).bytes;
}

int fmpnp_sp_nms_async(const float *heat, int H, int W, double conf_thresh, int nms_dist, int border, double *pts,
                       long long ld_pts, int *count_dev, int group, int *n_host, int *rounds_host, void *workspace,
                       size_t workspace_bytes, void *hip_stream) {
    const int rc = nms_args(heat, H, W, conf_thresh, nms_dist, border, pts, ld_pts);
    if (rc) return rc;
    if (!n_host || group < 1) return FMPNP_EINVAL;
    const NmsLayout l = nms_layout(H, W, nms_dist);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < l.bytes) return FMPNP_EINVAL;
    group = std::min(group, MAX_GROUP);
    hipStream_t s = (hipStream_t)hip_stream;
    // the pinned words the counts land in: a pool of their own, taken inside fmpnp_sp_nms's call on the other pool.
    // The stream is idle from each finish() to the resume() before the next piece of work is queued
    SyncCall pin(SCRATCH_SP_COUNTS, s, 0, 4 * N_COUNTERS, 0);
    if (pin.error()) return pin.error();
    volatile int *host = (volatile int *)pin.host;
    unsigned char *ws = (unsigned char *)workspace;
    uint64_t *words = (uint64_t *)(ws + l.o_words);
    unsigned char *state = ws + l.o_state;
    int *chunks = (int *)(ws + l.o_chunks), *counters = (int *)(ws + l.o_counters);
    const size_t HW = (size_t)H * (size_t)W;
    hipError_t e = hipMemsetAsync(counters, 0, 4 * N_COUNTERS, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nms_init_kernel, dim3((unsigned)((HW + SP_NT - 1) / SP_NT)), dim3(SP_NT), 0, s, heat, HW, (float)conf_thresh,
                       state, counters);
    const dim3 tiles((unsigned)((W + TX - 1) / TX), (unsigned)((H + TY - 1) / TY));
    long long rounds = 0;
    for (bool first = true;; first = false) {
        if (!first) {
            pin.resume();
            e = hipMemsetAsync(counters + CNT_LIVE, 0, 4 * (size_t)group, s);
            if (e != hipSuccess) return (int)e;
        }
        for (int r = 0; r < group; ++r) {
            hipLaunchKernelGGL(nms_round_kernel<0>, tiles, dim3(SP_NT), 0, s, heat, H, W, nms_dist, state, (int *)nullptr);
            hipLaunchKernelGGL(nms_round_kernel<1>, tiles, dim3(SP_NT), 0, s, heat, H, W, nms_dist, state,
                               counters + CNT_LIVE + r);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync((void *)host, counters, 4 * N_COUNTERS, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return (int)e;
        e = (hipError_t)pin.finish();
        if (e != hipSuccess) return (int)e;
        int done = -1;
        for (int r = 0; r < group && done < 0; ++r)
            if (host[CNT_LIVE + r] == 0) done = r;
        if (done >= 0) {
            rounds = host[CNT_CAND] ? rounds + done + 1 : 0;
            break;
        }
        rounds += group;
        if (rounds > (long long)host[CNT_CAND]) return FMPNP_EINVAL;  // (every round settles a candidate: unreachable)
    }
    pin.resume();
    hipLaunchKernelGGL(nms_count_kernel, dim3((unsigned)l.n_chunks), dim3(SP_NT), 0, s, state, HW, W, H, border, chunks);
    hipLaunchKernelGGL(nms_compact_kernel, dim3((unsigned)l.n_chunks), dim3(SP_NT), 0, s, state, heat, HW, W, H, border, chunks,
                       words, l.cap, counters, count_dev);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync((void *)host, counters, 4 * N_COUNTERS, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    e = (hipError_t)pin.finish();  // (the sort below is the caller's to wait for: it reads no pinned word)
    if (e != hipSuccess) return (int)e;
    const int n = host[CNT_KEPT];
    if (n < 0 || (long long)n > l.cap) return FMPNP_EINVAL;  // (unreachable: one kept point per cell at most)
    if (n > FMPNP_SP_MAX_KEYPOINTS) return FMPNP_ETOOBIG;
    if (n) {
        hipLaunchKernelGGL(nms_sort_kernel, dim3((unsigned)((n + SP_NT - 1) / SP_NT)), dim3(SP_NT), 0, s, words, n, heat, W, pts,
                           ld_pts);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    *n_host = n;
    if (rounds_host) *rounds_host = (int)rounds;
    return 0;
}

int fmpnp_sp_nms(const float *heat, int H, int W, double conf_thresh, int nms_dist, int border, double *pts_host,
                 long long ld_pts, int group, int *n_host, int *rounds_host, void *hip_stream) {
    const int rc0 = nms_args(heat, H, W, conf_thresh, nms_dist, border, pts_host, ld_pts);
    if (rc0) return rc0;
    if (!n_host || group < 1) return FMPNP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    const NmsLayout l = nms_layout(H, W, nms_dist);
    const size_t b_pts = align256(24 * (size_t)l.cap);
    SyncCall call(SCRATCH_SUPERPOINT, s, b_pts + l.bytes, 0);
    if (call.error()) return call.error();
    int n = 0;
    const int rc = fmpnp_sp_nms_async(heat, H, W, conf_thresh, nms_dist, border, (double *)call.dev, l.cap, nullptr, group,
                                      &n, rounds_host, call.dev + b_pts, l.bytes, hip_stream);
    if (rc) return rc;
    if (n) {
        const hipError_t e = hipMemcpy2DAsync(pts_host, 8 * (size_t)ld_pts, call.dev, 8 * (size_t)l.cap, 8 * (size_t)n, 3,
                                              hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return (int)e;
    }
    const int e = call.finish();
    if (e) return e;
    *n_host = n;
    return 0;
}

int fmpnp_sp_describe_async(const float *coarse, int D, int Hc, int Wc, const double *pts, long long ld_pts, int N,
                            int H, int W, int align_corners, float *desc, long long ld_desc, void *hip_stream) {
    const int rc = desc_args(coarse, D, Hc, Wc, pts, ld_pts, N, H, W, align_corners, desc, ld_desc);
    if (rc) return rc;
    if (!N) return 0;
    hipLaunchKernelGGL(sp_desc_kernel, dim3((unsigned)((N + SP_WAVES - 1) / SP_WAVES)), dim3(SP_NT), 0, (hipStream_t)hip_stream,
                       coarse, D, Hc, Wc, pts, ld_pts, N, H, W, align_corners, desc, ld_desc);
    return (int)hipGetLastError();
}

int fmpnp_sp_describe(const float *coarse, int D, int Hc, int Wc, const double *pts, long long ld_pts, int N, int H,
                      int W, int align_corners, float *desc_host, long long ld_desc, void *hip_stream) {
    const int rc0 = desc_args(coarse, D, Hc, Wc, pts, ld_pts, N, H, W, align_corners, desc_host, ld_desc);
    if (rc0) return rc0;
    if (!N) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    SyncCall call(SCRATCH_SUPERPOINT, s, 4 * (size_t)D * (size_t)N, 0);
    if (call.error()) return call.error();
    const int rc = fmpnp_sp_describe_async(coarse, D, Hc, Wc, pts, ld_pts, N, H, W, align_corners, (float *)call.dev, N,
                                           hip_stream);
    if (rc) return rc;
    const hipError_t e = hipMemcpy2DAsync(desc_host, 4 * (size_t)ld_desc, call.dev, 4 * (size_t)N, 4 * (size_t)N, (size_t)D,
                                          hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    return call.finish();
}

int fmpnp_sp_match_async(const float *desc1, int N1, int ld1, const float *desc2_t, int D, int N2, int ld2,
                         double ratio, int *nn_idx, float *nn_dist, unsigned char *ok, long long *matches, int *count,
                         void *workspace, size_t workspace_bytes, void *hip_stream) {
    const int rc = match_args(desc1, N1, ld1, desc2_t, D, N2, ld2, ratio, nn_idx, nn_dist, ok, matches, count);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!N1) return (int)hipMemsetAsync(count, 0, 4, s);
    const size_t need = fmpnp_match_workspace_size(N1, N2);
    if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need) return FMPNP_EINVAL;
    const int chunk = (int)(need / (4 * (size_t)N2));  // the rows of one round
    const float ratio2 = ratio_squared(ratio);
    for (int i0 = 0; i0 < N1; i0 += chunk) {  // (stream order: a round's reduction reads before the next round writes)
        const int n = std::min(chunk, N1 - i0);
        hipError_t e = launch_corr(desc1 + (size_t)i0 * ld1, n, ld1, desc2_t, D, N2, ld2, (float *)workspace, (size_t)N2, s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(nn2_kernel, dim3((unsigned)n), dim3(SP_NT), 0, s, (const float *)workspace, (size_t)N2, N2, ratio2,
                           nn_idx + 2 * (size_t)i0, nn_dist + 2 * (size_t)i0, ok + i0);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(compact_matches_kernel, dim3(1), dim3(SP_NT), 0, s, ok, nn_idx, N1, matches, count);
    return (int)hipGetLastError();
}

int fmpnp_sp_match(const float *desc1, int N1, int ld1, const float *desc2_t, int D, int N2, int ld2, double ratio,
                   int *nn_idx_host, float *nn_dist_host, unsigned char *ok_host, long long *matches_host,
                   int *count_host, void *hip_stream) {
    const int rc0 = match_args(desc1, N1, ld1, desc2_t, D, N2, ld2, ratio, nn_idx_host, nn_dist_host, ok_host, matches_host,
                               count_host);
    if (rc0) return rc0;
    if (!N1) {
        *count_host = 0;
        return 0;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t n1 = (size_t)N1, b_ws = align256(fmpnp_match_workspace_size(N1, N2));
    const size_t o_idx = b_ws, o_dist = o_idx + align256(8 * n1), o_ok = o_dist + align256(8 * n1), o_m = o_ok + align256(n1);
    const size_t o_cnt = o_m + align256(16 * n1), total = o_cnt + 256;
    SyncCall call(SCRATCH_SUPERPOINT, s, total, 256);
    if (call.error()) return call.error();
    unsigned char *d = call.dev;
    const int rc = fmpnp_sp_match_async(desc1, N1, ld1, desc2_t, D, N2, ld2, ratio, (int *)(d + o_idx), (float *)(d + o_dist),
                                        d + o_ok, (long long *)(d + o_m), (int *)(d + o_cnt), d, b_ws, hip_stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(call.host, d + o_cnt, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nn_idx_host, d + o_idx, 8 * n1, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nn_dist_host, d + o_dist, 8 * n1, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ok_host, d + o_ok, n1, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    e = (hipError_t)call.finish();  // (the count: the stream is idle until the rows' copy below)
    if (e != hipSuccess) return (int)e;
    const int n = *(const int *)call.host;
    if (n < 0 || n > N1) return FMPNP_EINVAL;  // (unreachable)
    if (n) {
        call.resume();
        e = hipMemcpyAsync(matches_host, d + o_m, 16 * (size_t)n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = (hipError_t)call.finish();
        if (e != hipSuccess) return (int)e;
    }
    *count_host = n;
    return 0;
}

int fmpnp_sp_assemble_async(const double *query_pts, int N1, long long ld_q, const double *ref_pts, int N2,
                            long long ld_r, const double *points2d, const double *points3d, int M,
                            const long long *matches, int n_matches, int *argmin, double *x2d, double *x2d_ref,
                            double *x3d, int *count, void *workspace, size_t workspace_bytes, void *hip_stream) {
    const int rc = assemble_args(query_pts, N1, ld_q, ref_pts, N2, ld_r, points2d, points3d, M, matches, n_matches, argmin,
                                 x2d, x2d_ref, x3d, count);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!N2) return (int)hipMemsetAsync(count, 0, 4, s);
    if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < 4 * (size_t)N2) return FMPNP_EINVAL;
    int *first = (int *)workspace;
    hipLaunchKernelGGL(closest_kernel, dim3((unsigned)((N2 + SP_WAVES - 1) / SP_WAVES)), dim3(SP_NT), 0, s, ref_pts, N2, ld_r,
                       points2d, M, argmin, first);
    if (n_matches)
        hipLaunchKernelGGL(first_match_kernel, dim3((unsigned)((n_matches + SP_NT - 1) / SP_NT)), dim3(SP_NT), 0, s, matches,
                           n_matches, N1, N2, first);
    hipLaunchKernelGGL(assemble_kernel, dim3(1), dim3(SP_NT), 0, s, query_pts, ld_q, ref_pts, N2, ld_r, points3d, argmin, first,
                       x2d, x2d_ref, x3d, count);
    return (int)hipGetLastError();
}

int fmpnp_sp_assemble(const double *query_pts, int N1, long long ld_q, const double *ref_pts, int N2, long long ld_r,
                      const double *points2d, const double *points3d, int M, const long long *matches, int n_matches,
                      int *argmin_host, double *x2d_host, double *x2d_ref_host, double *x3d_host, int *count_host,
                      void *hip_stream) {
    const int rc0 = assemble_args(query_pts, N1, ld_q, ref_pts, N2, ld_r, points2d, points3d, M, matches, n_matches,
                                  argmin_host, x2d_host, x2d_ref_host, x3d_host, count_host);
    if (rc0) return rc0;
    if (!N2) {
        *count_host = 0;
        return 0;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t n2 = (size_t)N2;
    const size_t o_first = 0, o_arg = align256(4 * n2), o_x2 = o_arg + align256(4 * n2), o_r2 = o_x2 + align256(16 * n2);
    const size_t o_x3 = o_r2 + align256(16 * n2), o_cnt = o_x3 + align256(24 * n2), total = o_cnt + 256;
    SyncCall call(SCRATCH_SUPERPOINT, s, total, 256);
    if (call.error()) return call.error();
    unsigned char *d = call.dev;
    const int rc = fmpnp_sp_assemble_async(query_pts, N1, ld_q, ref_pts, N2, ld_r, points2d, points3d, M, matches, n_matches,
                                           (int *)(d + o_arg), (double *)(d + o_x2), (double *)(d + o_r2),
                                           (double *)(d + o_x3), (int *)(d + o_cnt), d + o_first, 4 * n2, hip_stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(call.host, d + o_cnt, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(argmin_host, d + o_arg, 4 * n2, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return (int)e;
    e = (hipError_t)call.finish();  // (the count: the stream is idle until the rows' copy below)
    if (e != hipSuccess) return (int)e;
    const int n = *(const int *)call.host;
    if (n < 0 || n > N2) return FMPNP_EINVAL;  // (unreachable)
    if (n) {
        call.resume();
        e = hipMemcpyAsync(x2d_host, d + o_x2, 16 * (size_t)n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(x2d_ref_host, d + o_r2, 16 * (size_t)n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(x3d_host, d + o_x3, 24 * (size_t)n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = (hipError_t)call.finish();
        if (e != hipSuccess) return (int)e;
    }
    *count_host = n;
    return 0;
}

}  // extern "C"
