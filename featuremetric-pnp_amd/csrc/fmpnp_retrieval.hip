// fmpnp_retrieval.hip -- the retrieval stage on gfx950: NetVLAD pooling (s2dhm/network/netvlad.py:45-70)
// and the top-n reference ranking (s2dhm/image_retrieval/rank_images.py:81-84).  include/fmpnp.h states
// the numeric contract; csrc/fmpnp_retrieval_impl.h holds the arithmetic shared with the CPU twin.
//
//   assign_kernel     a workgroup owns 64 positions of one image: their norms, the logits
//                     W [K x C] . x^ [C x 64] on v_mfma_f32_32x32x2_f32 (each logit one fmaf chain over c
//                     ascending from +0; the zero-padded tail adds fma(0, 0, acc)), and the softmax over
//                     the clusters.  It writes the assignments a [K][P] and the denominators d [P].
//   aggregate_kernel  a workgroup owns a 64 x 128 tile of one segment's partial
//                     V_s[k][c] = sum_{p in segment} a[k][p] . x^[c][p], the same MFMA with the positions
//                     as the reduction index, ascending; channel tile 0 also adds up the assignment sum
//                     (the same chain with x^ = 1: fma(a, 1, acc) = acc + a) into column C of the partial.
//                     A segment is FMPNP_NETVLAD_SEGMENT positions whatever the launch, and a partial is
//                     written by exactly one workgroup: no split, no atomics.
//   rownorm_kernel    one wave per (image, cluster): the partials added in segment order, the centroid
//                     term, the intra-normalisation, and the row's share of the final sum of squares.
//   scale_kernel      the final normalisation.
//   rank_kernel       one workgroup per query row of the score map (launch_corr's): a radix select of the
//                     n-th greatest (key, index) word, the n words at or above it compacted into LDS and
//                     sorted there.  The words are distinct, so the LDS atomics that place them change no
//                     result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fmpnp.h"
#include "fmpnp_internal.h"
#include "fmpnp_retrieval_impl.h"

namespace fmpnp {

namespace {

using namespace rv;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RV_NT = 256;  // 4 waves
constexpr int TK = 32;   // reduction indices per LDS tile
constexpr int LB = 8;    // loads issued together ahead of a chain's links (latency; no effect on a value)

// ---- assignments --------------------------------------------------------------------------------
constexpr int A_BM = 64, A_BN = 64;  // clusters x positions per accumulator round; wave w: 32 x 32 at (w >> 1, w & 1)
constexpr int A_WLD = A_BM + 1;      // W tile, c-major and transposed on the way in: odd stride

__global__ __launch_bounds__(RV_NT) void assign_kernel(const float *__restrict__ x, size_t sb, size_t sc, int C, int P,
                                                    const float *__restrict__ w, int K, int ld_w, int normalize,
                                                    float *a, float *__restrict__ d) {
    __shared__ float Ws[TK * A_WLD];
    __shared__ float Xs[TK * A_BN];
    __shared__ float s_part[NORM_CHAINS][A_BN];
    __shared__ float s_d[A_BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * A_BN;
    const size_t img = blockIdx.y;
    const float *xb = x + img * sb;
    float *ab = a + img * (size_t)K * (size_t)P;
    const int pl = tid & 63, q = tid >> 6;  // position of the tile, chain / cluster quarter
    const int p = p0 + pl;
    // the denominators: chain q takes c = q, q + 4, ... ascending
    if (normalize) {
        float s = 0.f;
        if (p < P)
            for (int c = q; c < C; c += NORM_CHAINS * LB) {  // LB loads in flight, then their links in order
                float v[LB];
#pragma unroll
                for (int u = 0; u < LB; ++u) {
                    const int cc = c + NORM_CHAINS * u;
                    v[u] = cc < C ? xb[(size_t)cc * sc + p] : 0.f;  // (fma(0, 0, s) = s: s is never -0)
                }
#pragma unroll
                for (int u = 0; u < LB; ++u) s = square_link(v[u], s);
            }
        s_part[q][pl] = s;
        __syncthreads();
        if (tid < A_BN) {
            const float dd = position_norm(s_part[0][tid], s_part[1][tid], s_part[2][tid], s_part[3][tid]);
            s_d[tid] = dd;
            if (p < P) d[img * (size_t)P + p] = dd;
        }
    } else if (tid < A_BN) {
        s_d[tid] = 1.f;
    }
    __syncthreads();
    // the logits, 64 clusters per round
    const int w_c = tid & 31, w_m = tid >> 5;  // W element e: (m = e * 8 + w_m, c = w_c)
    const int x_n = tid & 63, x_c = tid >> 6;  // x element e: (c = e * 4 + x_c, n = x_n)
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int r = lane & 31, h = lane >> 5;
    const float dn = s_d[x_n];
    constexpr int W_PER_T = A_BM * TK / RV_NT, X_PER_T = TK * A_BN / RV_NT;  // 8 and 8
    float rw[W_PER_T], rx[X_PER_T];
    for (int kb = 0; kb < K; kb += A_BM) {
        // global -> register staging (out-of-range elements are zero); x is divided on its way into LDS
        auto fetch = [&](int c0) {
#pragma unroll
            for (int e = 0; e < W_PER_T; ++e) {
                const int m = kb + e * 8 + w_m, c = c0 + w_c;
                rw[e] = (m < K && c < C) ? w[(size_t)m * ld_w + c] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < X_PER_T; ++e) {
                const int c = c0 + e * 4 + x_c, n = p0 + x_n;
                rx[e] = (c < C && n < P) ? xb[(size_t)c * sc + n] : 0.f;
            }
        };
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = 0.f;
        fetch(0);
        for (int c0 = 0; c0 < C; c0 += TK) {
            __syncthreads();  // the previous tile's reads are done
#pragma unroll
            for (int e = 0; e < W_PER_T; ++e) Ws[w_c * A_WLD + e * 8 + w_m] = rw[e];
#pragma unroll
            for (int e = 0; e < X_PER_T; ++e) {
                const bool in = c0 + e * 4 + x_c < C && p0 + x_n < P;
                Xs[(e * 4 + x_c) * A_BN + x_n] = (in && normalize) ? quotient(rx[e], dn) : rx[e];
            }
            __syncthreads();
            if (c0 + TK < C) fetch(c0 + TK);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
            for (int kk = 0; kk < TK; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[(kk + h) * A_WLD + wm + r], Xs[(kk + h) * A_BN + wn + r],
                                                           acc, 0, 0, 0);
        }
        // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const int col = p0 + wn + r;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = kb + wm + (g & 3) + 8 * (g >> 2) + 4 * h;
            if (row < K && col < P) ab[(size_t)row * P + col] = acc[g];
        }
    }
    __syncthreads();  // (the block's own logits are visible to all of it)
    // the softmax over the clusters of each position: quarter q takes k = q, q + 4, ...
    float m = __uint_as_float(0x7fc00000u);  // (NaN: max_link ignores it)
    float *col = ab + p;
    const size_t ldk = (size_t)P;
    if (p < P)
        for (int k = q; k < K; k += 4 * LB) {
            float v[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) v[u] = k + 4 * u < K ? col[(size_t)(k + 4 * u) * ldk] : m;
#pragma unroll
            for (int u = 0; u < LB; ++u) m = max_link(m, v[u]);
        }
    s_part[q][pl] = m;
    __syncthreads();
    m = max_link(max_link(s_part[0][pl], s_part[1][pl]), max_link(s_part[2][pl], s_part[3][pl]));
    if (p < P)
        for (int k = q; k < K; k += 4 * LB) {
            float v[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) v[u] = k + 4 * u < K ? col[(size_t)(k + 4 * u) * ldk] : 0.f;
#pragma unroll
            for (int u = 0; u < LB; ++u)
                if (k + 4 * u < K) col[(size_t)(k + 4 * u) * ldk] = exp_neg(v[u] - m);
        }
    __syncthreads();
    if (tid < A_BN) {  // the sum: one chain over k ascending from +0
        float s = 0.f;
        if (p < P)
            for (int k = 0; k < K; k += 2 * LB) {
                float v[2 * LB];
#pragma unroll
                for (int u = 0; u < 2 * LB; ++u) v[u] = k + u < K ? col[(size_t)(k + u) * ldk] : 0.f;
#pragma unroll
                for (int u = 0; u < 2 * LB; ++u)
                    if (k + u < K) s = s + v[u];
            }
        s_d[tid] = s;
    }
    __syncthreads();
    const float sum = s_d[pl];
    if (p < P)
        for (int k = q; k < K; k += 4 * LB) {
            float v[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) v[u] = k + 4 * u < K ? col[(size_t)(k + 4 * u) * ldk] : 0.f;
#pragma unroll
            for (int u = 0; u < LB; ++u)
                if (k + 4 * u < K) col[(size_t)(k + 4 * u) * ldk] = quotient(v[u], sum);
        }
}

// ---- aggregation --------------------------------------------------------------------------------
constexpr int G_BM = 64, G_BN = 128;  // clusters x channels per workgroup; wave w: 32 x 64 at (w >> 1, w & 1)
constexpr int G_ALD = G_BM + 1, G_BLD = G_BN + 1;  // both tiles are written transposed (lanes run along p)
constexpr int G_A_PER_T = G_BM * TK / RV_NT, G_B_PER_T = TK * G_BN / RV_NT;  // 8 and 16

__global__ __launch_bounds__(RV_NT) void aggregate_kernel(const float *__restrict__ x, size_t sb, size_t sc, int C, int P,
                                                       int K, int normalize, const float *__restrict__ a,
                                                       const float *__restrict__ d, float *__restrict__ part,
                                                       int col_tiles, int nseg) {
    __shared__ float As[TK * G_ALD];
    __shared__ float Bs[TK * G_BLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ct = blockIdx.x % col_tiles, kt = blockIdx.x / col_tiles;
    const int seg = blockIdx.y;
    const size_t img = blockIdx.z;
    const int kb = kt * G_BM, cb = ct * G_BN;
    const int ps = seg * SEG, pe = min(P, ps + SEG);
    const float *xb = x + img * sb;
    const float *ab = a + img * (size_t)K * (size_t)P;
    const float *db = d + img * (size_t)P;
    const int t_p = tid & 31, t_j = tid >> 5;  // element e of either tile: (row or column e * 8 + t_j, position t_p)
    float ra[G_A_PER_T], rb[G_B_PER_T];
    auto fetch = [&](int q0) {
        const int p = q0 + t_p;
        const bool in = p < pe;
        const float dn = (in && normalize) ? db[p] : 1.f;
#pragma unroll
        for (int e = 0; e < G_A_PER_T; ++e) {
            const int k = kb + e * 8 + t_j;
            ra[e] = (in && k < K) ? ab[(size_t)k * P + p] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < G_B_PER_T; ++e) {
            const int c = cb + e * 8 + t_j;
            float v = 0.f;
            if (in && c < C) {
                v = xb[(size_t)c * sc + p];
                if (normalize) v = quotient(v, dn);
            }
            rb[e] = v;
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[b][g] = 0.f;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    // the assignment sums S_j[k] = acc + a[k][p] over the segment's positions ascending (the chain
    // fma(a, 1, acc) of the contract), by the first 64 threads of channel tile 0 from the a tile in LDS
    const bool sums = ct == 0 && tid < G_BM;
    float s_acc = 0.f;
    fetch(ps);
    for (int q0 = ps; q0 < pe; q0 += TK) {
        __syncthreads();  // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < G_A_PER_T; ++e) As[t_p * G_ALD + e * 8 + t_j] = ra[e];
#pragma unroll
        for (int e = 0; e < G_B_PER_T; ++e) Bs[t_p * G_BLD + e * 8 + t_j] = rb[e];
        __syncthreads();
        if (q0 + TK < pe) fetch(q0 + TK);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < TK; kk += 2) {
            const float av = As[(kk + h) * G_ALD + wm + r];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Bs[(kk + h) * G_BLD + wn + r], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Bs[(kk + h) * G_BLD + wn + 32 + r], acc[1], 0, 0, 0);
        }
        if (sums) {  // (rows beyond K and positions beyond the segment are zeros in the tile)
#pragma unroll
            for (int kk = 0; kk < TK; ++kk) s_acc = s_acc + As[kk * G_ALD + tid];
        }
    }
    const size_t ldp = (size_t)C + 1;
    float *pb = part + ((img * (size_t)nseg + (size_t)seg) * (size_t)K) * ldp;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col = cb + wn + b * 32 + r;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = kb + wm + (g & 3) + 8 * (g >> 2) + 4 * h;
            if (row < K && col < C) pb[(size_t)row * ldp + col] = acc[b][g];
        }
    }
    if (sums && kb + tid < K) pb[(size_t)(kb + tid) * ldp + C] = s_acc;
}

// ---- finalisation -------------------------------------------------------------------------------
__device__ inline float tree64(float v) {  // t[i] += t[i + o] for o = 32 .. 1: every lane ends with t[0]
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void rownorm_kernel(const float *__restrict__ part, int nseg, int K, int C,
                                                     const float *__restrict__ cent, int ld_c, float *out,
                                                     size_t ld_out, float *__restrict__ tk) {
    const int lane = threadIdx.x, k = blockIdx.x;
    const size_t img = blockIdx.y;
    const size_t ldp = (size_t)C + 1, seg_stride = (size_t)K * ldp;
    const float *pb = part + img * (size_t)nseg * seg_stride + (size_t)k * ldp;
    float *row = out + img * ld_out + (size_t)k * (size_t)C;
    // sum of one column's partials in segment order, LB loads in flight at a time
    auto column = [&](int c) {
        float t = 0.f;
        for (int s = 0; s < nseg; s += LB) {
            float v[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) v[u] = s + u < nseg ? pb[(size_t)(s + u) * seg_stride + c] : 0.f;
#pragma unroll
            for (int u = 0; u < LB; ++u)
                if (s + u < nseg) t = t + v[u];
        }
        return t;
    };
    const float S = column(C);
    float ss = 0.f;  // chain `lane` takes c = lane, lane + 64, ... ascending
    for (int c = lane; c < C; c += ROW_CHAINS) {
        const float V = column(c);
        const float v = centroid_term(V, S, cent[(size_t)k * ld_c + c]);
        row[c] = v;
        ss = square_link(v, ss);
    }
    const float n = norm_floor(tree64(ss));
    float t = 0.f;
    for (int c = lane; c < C; c += ROW_CHAINS) {
        const float v = quotient(row[c], n);  // (this lane's own store)
        row[c] = v;
        t = square_link(v, t);
    }
    t = tree64(t);
    if (lane == 0) tk[img * (size_t)K + k] = t;
}

__global__ __launch_bounds__(RV_NT) void scale_kernel(float *out, size_t ld_out, int KC, int K,
                                                   const float *__restrict__ tk) {
    const size_t img = blockIdx.y;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = s + tk[img * (size_t)K + k];  // ascending k from +0
    const float n = norm_floor(s);
    float *row = out + img * ld_out;
    const int i0 = blockIdx.x * (RV_NT * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * RV_NT + (int)threadIdx.x;
        if (i < KC) row[i] = quotient(row[i], n);
    }
}

// ---- ranking ------------------------------------------------------------------------------------
constexpr int RK_NT = 256;

__global__ __launch_bounds__(RK_NT) void rank_kernel(const float *__restrict__ scores, size_t ld_scores, int R, int n,
                                                     int *__restrict__ idx, float *__restrict__ top) {
    __shared__ unsigned hist[256], scan[256];
    __shared__ unsigned long long buf[RANK_CAP];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_want, s_count;
    const int tid = threadIdx.x;
    const float *row = scores + (size_t)blockIdx.x * ld_scores;
    unsigned long long prefix = 0;  // the decided high bytes of the n-th greatest word
    unsigned want = (unsigned)n;    // it is the want-th greatest among the words matching prefix
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < R; j += RK_NT) {
            const unsigned long long wd = rank_word(row[j], (unsigned)j);
            if (pass == 0 || (wd >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(wd >> shift) & 255u], 1u);
        }
        __syncthreads();
        scan[tid] = hist[tid];  // -> scan[b] = the count of bins b .. 255
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned v = tid + off < 256 ? scan[tid + off] : 0u;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const unsigned incl = scan[tid], excl = incl - hist[tid];
        if (excl < want && want <= incl) {  // (exactly one bin)
            s_prefix = prefix | ((unsigned long long)tid << shift);
            s_want = want - excl;
        }
        __syncthreads();
        prefix = s_prefix;
        want = s_want;
        __syncthreads();
    }
    // the words are distinct: exactly n of them are >= prefix
    int npad = 1;
    while (npad < n) npad <<= 1;
    if (tid == 0) s_count = 0;
    for (int i = tid; i < npad; i += RK_NT) buf[i] = 0ull;  // (a real word is never 0: its index bits are ~j)
    __syncthreads();
    for (int j = tid; j < R; j += RK_NT) {
        const unsigned long long wd = rank_word(row[j], (unsigned)j);
        if (wd >= prefix) {
            const unsigned slot = atomicAdd(&s_count, 1u);
            if (slot < (unsigned)n) buf[slot] = wd;
        }
    }
    __syncthreads();
    // bitonic sort, descending
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += RK_NT) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long u = buf[i], v = buf[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? u < v : u > v) {
                        buf[i] = v;
                        buf[l] = u;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += RK_NT) {
        const unsigned j = word_index(buf[i]);
        idx[(size_t)blockIdx.x * n + i] = (int)j;
        top[(size_t)blockIdx.x * n + i] = row[j];
    }
}

constexpr size_t POOL_WS_CAP = (size_t)64 << 20;  // workspace of a round of images (one image at least)

struct PoolWs {
    size_t a, d, part, tk, per_image;
    int nseg;
};
inline PoolWs pool_ws(int K, int C, int P) {
    PoolWs s;
    s.nseg = (P + SEG - 1) / SEG;
    s.a = align256(sizeof(float) * (size_t)K * (size_t)P);
    s.d = align256(sizeof(float) * (size_t)P);
    s.part = align256(sizeof(float) * (size_t)s.nseg * (size_t)K * ((size_t)C + 1));
    s.tk = align256(sizeof(float) * (size_t)K);
    s.per_image = s.a + s.d + s.part + s.tk;
    return s;
}
inline int pool_round(int B, const PoolWs &s) {
    const size_t n = std::max<size_t>(1, POOL_WS_CAP / s.per_image);
    return (int)std::min<size_t>(std::min<size_t>(n, 32768), (size_t)std::max(B, 1));
}

}  // namespace

size_t netvlad_workspace_bytes(int B, int K, int C, int P) {
    const PoolWs s = pool_ws(K, C, P);
    return (size_t)pool_round(B, s) * s.per_image;
}

int launch_netvlad_pool(const float *x, int B, int C, int P, long long sb, long long sc, const float *w, int K, int ld_w,
                        const float *cent, int ld_c, int normalize, float *out, long long ld_out, void *workspace,
                        hipStream_t s) {
    const PoolWs ws = pool_ws(K, C, P);
    const int round = pool_round(B, ws);
    const long long p_tiles = (P + A_BN - 1) / A_BN;
    const long long col_tiles = ((long long)C + G_BN - 1) / G_BN, k_tiles = (K + G_BM - 1) / G_BM;
    const long long s_tiles = ((long long)K * C + RV_NT * 4 - 1) / (RV_NT * 4);
    if (col_tiles * k_tiles > INT32_MAX || ws.nseg > 65535) return FMPNP_ETOOBIG;  // (pool_args rules both out)
    unsigned char *base = (unsigned char *)workspace;
    for (int b0 = 0; b0 < B; b0 += round) {  // (stream order: a round's kernels read before the next round writes)
        const unsigned nb = (unsigned)std::min(round, B - b0);
        float *a = (float *)base, *d = (float *)(base + nb * ws.a);
        float *part = (float *)(base + nb * (ws.a + ws.d)), *tk = (float *)(base + nb * (ws.a + ws.d + ws.part));
        const float *xr = x + (size_t)b0 * (size_t)sb;
        float *outr = out + (size_t)b0 * (size_t)ld_out;
        hipLaunchKernelGGL(assign_kernel, dim3((unsigned)p_tiles, nb), dim3(RV_NT), 0, s, xr, (size_t)sb, (size_t)sc, C, P,
                           w, K, ld_w, normalize, a, d);
        hipLaunchKernelGGL(aggregate_kernel, dim3((unsigned)(col_tiles * k_tiles), (unsigned)ws.nseg, nb), dim3(RV_NT), 0,
                           s, xr, (size_t)sb, (size_t)sc, C, P, K, normalize, a, d, part, (int)col_tiles, ws.nseg);
        // (K rows per image: up to 65535 images per launch in y, so the rows go in x)
        hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)K, nb), dim3(64), 0, s, part, ws.nseg, K, C, cent, ld_c, outr,
                           (size_t)ld_out, tk);
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)s_tiles, nb), dim3(RV_NT), 0, s, outr, (size_t)ld_out, K * C, K, tk);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

hipError_t launch_rank(const float *scores, size_t ld_scores, int Q, int R, int n, int *idx, float *top,
                       hipStream_t s) {
    hipLaunchKernelGGL(rank_kernel, dim3((unsigned)Q), dim3(RK_NT), 0, s, scores, ld_scores, R, n, idx, top);
    return hipGetLastError();
}

}  // namespace fmpnp
