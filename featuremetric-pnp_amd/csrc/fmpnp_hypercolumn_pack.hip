// fmpnp_hypercolumn_pack.hip -- the fused hypercolumn pack (fmpnp_hypercolumn_pack*): the encoder's layers go
// straight into the refiner's packed layout, [H][W][3][cstride] = (f, gx, gy) or [H][W][cstride] = f, without
// the dense [C][H][W] hypercolumn in between.  include/fmpnp.h states the contract: every element written is
// the one fmpnp_hypercolumn_assemble followed by fmpnp_pack_features / fmpnp_pack_features_f writes, bit for
// bit.  Every value is formed by the functions of fmpnp_hypercolumn_impl.h (taps, bilerp, the fp64 block sums,
// the division) and fmpnp_hypercolumn_pack_impl.h (the Sobel's association, the padding), which the CPU twin
// calls too.  Built with -ffp-contract=off.
//
// Two kernels:
//   hc_norm_kernel  pass 1 of the assembly kernel: n = (float)sqrt(sum of squares over ALL concatenated
//                   channels) per texel, one fp32 per texel into an H x W plane.  It does not depend on the
//                   channel range, so a caller that packs a map in several ranges forms it once.
//   hc_pack_kernel  the Sobel pack's pipeline (fmpnp_pack.hip sobel_pack_kernel: a tile of 64 channels x 32
//                   columns x rs rows, input rows in a 4-slot LDS ring of odd row stride, lane = channel in the
//                   compute phase, 256 contiguous bytes per plane store, tiles without a mark skipped) with
//                   another row source: instead of copying a CHW row into the ring, the loader FORMS it, lanes
//                   along x -- the four taps of the layer that owns each channel, the nine fp32 operations and
//                   the division by the texel's n.  The taps of row y + 2 are loaded into registers before row
//                   y is computed and turned into values after it, so their latency hides under the Sobel and
//                   its stores.  A value is formed once per tile (plus the halo) and divided once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_hypercolumn_pack_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {
namespace {

using namespace hc;
using namespace hcp;

struct HpLayers {
    fmpnp_hc_layer layer[MAX_LAYERS];  // data: the batch item's channel 0
    int L, H, W, C;
};

// ---- the norm plane --------------------------------------------------------------------------------------
// One workgroup of 4 waves per 64 texels of a row; the 64-channel blocks are dealt over the waves and meet in
// LDS after every round of 4, where each wave adds them to its own running sum in ascending block order (the
// assembly kernel's scheme with half the waves).
constexpr int HN_NW = 4, HN_NT = 64 * HN_NW;

struct HnArgs {
    HpLayers m;
    float *norm;
    const unsigned char *marks;  // NULL, or [H][W]: tiles without a mark within one texel are skipped
    int nblocks;
    unsigned tiles_x;
};

__global__ __launch_bounds__(HN_NT) void hc_norm_kernel(const HnArgs a) {
    __shared__ double part[2][HN_NW][64];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int H = a.m.H, W = a.m.W;
    const int y = (int)(blockIdx.x / a.tiles_x), x0 = (int)(blockIdx.x % a.tiles_x) * 64;
    const int x = x0 + lane, xc = min(x, W - 1);  // (a lane past the row's end repeats its last texel)
    if (a.marks) {
        int any = 0;
        for (int e = (int)threadIdx.x; e < 3 * 66; e += HN_NT) {
            const int yy = y - 1 + e / 66, xx = x0 - 1 + e % 66;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) any |= a.marks[(size_t)yy * W + xx];
        }
        if (!__syncthreads_or(any)) return;
    }
    double sum = 0.0;
    for (int r0 = 0, r = 0; r0 < a.nblocks; r0 += HN_NW, ++r) {
        const int blk = r0 + wave;
        double acc = 0.0;
        if (blk < a.nblocks) {
            const int c_lo = blk * BLOCK, c_hi = min(a.m.C, c_lo + BLOCK);
            int first = 0;
            for (int l = 0; l < a.m.L && first < c_hi; ++l) {
                const fmpnp_hc_layer &ly = a.m.layer[l];
                const int lo = max(c_lo, first), hi = min(c_hi, first + ly.C);
                if (lo < hi) {
                    const Tap ty = axis_tap(axis_scale(ly.H, H), ly.H, y);
                    const Tap tx = axis_tap(axis_scale(ly.W, W), ly.W, xc);
                    const size_t cs = (size_t)ly.stride_c;
                    const float *p0 = ly.data + (size_t)(lo - first) * cs + (size_t)ty.i0 * (size_t)ly.stride_y;
                    const float *p1 = ly.data + (size_t)(lo - first) * cs + (size_t)ty.i1 * (size_t)ly.stride_y;
#pragma unroll 4
                    for (int c = lo; c < hi; ++c, p0 += cs, p1 += cs) {
                        const float v = bilerp(p0[tx.i0], p0[tx.i1], p1[tx.i0], p1[tx.i1], tx.w0, tx.w1, ty.w0, ty.w1);
                        acc = square_acc(v, acc);
                    }
                }
                first += ly.C;
            }
        }
        // two buffers, one barrier per round: a wave writes round r + 2's partials only after the barrier of
        // round r + 1, which every wave reaches after it has read round r's
        double(*p)[64] = part[r & 1];
        p[wave][lane] = acc;
        __syncthreads();
        const int nb = min(HN_NW, a.nblocks - r0);
        for (int j = 0; j < nb; ++j) sum = sum + p[j][lane];
    }
    if (wave == 0 && x < W) a.norm[(size_t)y * W + x] = norm_of(sum);
}

// ---- the pack --------------------------------------------------------------------------------------------
constexpr int HP_NT = 256;
constexpr int HP_CB = 64;                  // channels per tile (one per lane in the compute phase)
constexpr int HP_XW = 32;                  // columns per tile (4 waves x 8-column runs)
constexpr int HP_RUN = HP_XW / (HP_NT / 64);
constexpr int HP_COLS = HP_XW + 2;         // with the halo columns
constexpr int HP_LD = HP_XW + 5;           // 37: odd, >= HP_COLS
constexpr int HP_SE = HP_CB * HP_LD;       // floats per ring slot
constexpr int HP_SLOTS = 4;
constexpr int HP_VALS = HP_CB * HP_COLS;   // values of one formed row: 2176
constexpr int HP_U = (HP_VALS + HP_NT - 1) / HP_NT;  // per thread: 9 (the last one in half the threads)

struct HpArgs {
    HpLayers m;
    const float *norm;           // the norm plane, or NULL: no normalisation
    const unsigned char *marks;  // WIN: [H][W]
    void *out;
    int c_begin, c_end, cs, rs, ncb, nxw, ntiles, replicate, sobel_normalized;
};

// what the loader needs of a layer, in LDS (indexed per lane: a chunk of 64 channels may straddle layers)
struct LayerTab {
    const float *data;
    size_t stride_c, stride_y;
    float sy, sx;
    int H, W, first;
};

// a thread's share of one formed row: unit i is value e = tid + 256 i of [64 channels][34 columns], lanes along x
struct HpUnits {
    const float *base[HP_U];  // the owning layer's channel plane
    int xo0[HP_U], xo1[HP_U], li[HP_U];
    float w1x[HP_U];
    unsigned okm;             // bit i: unit i is a channel of the range at a column that is no zero padding
};

struct HpRow {
    float t[HP_U][4], n[HP_U];
};

__device__ __forceinline__ int unit_index(int i) { return min((int)threadIdx.x + HP_NT * i, HP_VALS - 1); }

__device__ __forceinline__ void hp_units(HpUnits &u, const HpArgs &a, const LayerTab *tab, int c0, int x0) {
    u.okm = 0;
#pragma unroll
    for (int i = 0; i < HP_U; ++i) {
        const int e = unit_index(i), cc = e / HP_COLS, xx = e - cc * HP_COLS;
        const int c = min(c0 + cc, a.c_end - 1);  // (a lane past the range forms its last channel and drops it)
        int l = 0;
        while (l + 1 < a.m.L && c >= tab[l + 1].first) ++l;
        int xs;
        const bool col_ok = pad(x0 - 1 + xx, a.m.W, a.replicate != 0, &xs);
        const Tap tx = axis_tap(tab[l].sx, tab[l].W, xs);
        u.base[i] = tab[l].data + (size_t)(c - tab[l].first) * tab[l].stride_c;
        u.xo0[i] = tx.i0;
        u.xo1[i] = tx.i1;
        u.w1x[i] = tx.w1;
        u.li[i] = l;
        if (col_ok && c0 + cc < a.c_end && (int)threadIdx.x + HP_NT * i < HP_VALS) u.okm |= 1u << i;
    }
}

// issue the loads of row y: the taps and the texels' norms (no use of a loaded value here).  With a mark plane
// hc_norm_kernel writes the norms only where a mark lies within one texel, so a norm read here may be
// uninitialised memory: such a value only reaches texels further than one from every mark, none of which is stored
__device__ __forceinline__ void hp_load(HpRow &r, const HpUnits &u, const HpArgs &a, const LayerTab *tab, int x0, int y) {
    int ys;
    (void)pad(y, a.m.H, a.replicate != 0, &ys);
#pragma unroll
    for (int i = 0; i < HP_U; ++i) {
        const LayerTab &T = tab[u.li[i]];
        const Tap ty = axis_tap(T.sy, T.H, ys);
        const float *r0 = u.base[i] + (size_t)ty.i0 * T.stride_y, *r1 = u.base[i] + (size_t)ty.i1 * T.stride_y;
        r.t[i][0] = r0[u.xo0[i]];
        r.t[i][1] = r0[u.xo1[i]];
        r.t[i][2] = r1[u.xo0[i]];
        r.t[i][3] = r1[u.xo1[i]];
        if (a.norm) {
            const int e = unit_index(i), xx = e % HP_COLS;
            int xs;
            (void)pad(x0 - 1 + xx, a.m.W, a.replicate != 0, &xs);
            r.n[i] = a.norm[(size_t)ys * a.m.W + xs];
        }
    }
}

// form row y's values from the loaded taps and put them into the ring slot
__device__ __forceinline__ void hp_store(const HpRow &r, const HpUnits &u, const HpArgs &a, const LayerTab *tab, int y,
                                         float *slot) {
    int ys;
    const bool row_ok = pad(y, a.m.H, a.replicate != 0, &ys);
#pragma unroll
    for (int i = 0; i < HP_U; ++i) {
        const LayerTab &T = tab[u.li[i]];
        const Tap ty = axis_tap(T.sy, T.H, ys);
        float v = bilerp(r.t[i][0], r.t[i][1], r.t[i][2], r.t[i][3], 1.0f - u.w1x[i], u.w1x[i], ty.w0, ty.w1);
        if (a.norm) v = normalised(v, r.n[i]);
        const int e = unit_index(i), cc = e / HP_COLS, xx = e - cc * HP_COLS;
        if ((int)threadIdx.x + HP_NT * i < HP_VALS) slot[cc * HP_LD + xx] = (row_ok && ((u.okm >> i) & 1u)) ? v : 0.0f;
    }
}

template <typename Tout>
__device__ __forceinline__ void hp_put(Tout *p, Tout v) { __builtin_nontemporal_store(v, p); }

// the wave's run of 8 columns of row y, lane = channel: the Sobel pack's sliding 3 x 3 window
template <typename Tout, bool GRAD, bool WIN>
__device__ __forceinline__ void hp_row(const float *rm, const float *r0, const float *rp, Tout *o, size_t tstride,
                                       int cs, int ncols, unsigned wmask, bool sn) {
    if constexpr (GRAD) {
        const double am = rm[0], dm = r0[0], gm = rp[0];
        const double a1 = rm[1], d1 = r0[1], g1 = rp[1];
        double sxm = col_sx(am, dm, gm), sym = col_sy(am, gm);
        double sx0 = col_sx(a1, d1, g1), sy0 = col_sy(a1, g1);
        float f0 = r0[1];
#pragma unroll
        for (int k = 0; k < HP_RUN; ++k) {
            const double a2 = rm[k + 2], d2 = r0[k + 2], g2 = rp[k + 2];
            const double sxp = col_sx(a2, d2, g2), syp = col_sy(a2, g2);
            const double gx = grad_x(sxm, sxp), gy = grad_y(sym, sy0, syp);
            if (k < ncols && (!WIN || ((wmask >> k) & 1u))) {
                Tout *p = o + (size_t)k * tstride;
                hp_put<Tout>(p, (Tout)f0);
                hp_put<Tout>(p + cs, (Tout)scaled(gx, sn));
                hp_put<Tout>(p + 2 * cs, (Tout)scaled(gy, sn));
            }
            sxm = sx0; sym = sy0; sx0 = sxp; sy0 = syp; f0 = r0[k + 2];
        }
    } else {
#pragma unroll
        for (int k = 0; k < HP_RUN; ++k)
            if (k < ncols && (!WIN || ((wmask >> k) & 1u))) hp_put<Tout>(o + (size_t)k * tstride, (Tout)r0[k + 1]);
    }
}

template <typename Tout, bool GRAD, bool WIN>
__global__ __launch_bounds__(HP_NT) void hc_pack_kernel(const HpArgs a) {
    __shared__ float ring[HP_SLOTS * HP_SE];
    __shared__ LayerTab tab[MAX_LAYERS];
    const int H = a.m.H, W = a.m.W;
    // tile order as the Sobel pack's: channel chunk fastest, then column block, then row block; workgroup b
    // takes tile (b % 8) * (grid / 8) + b / 8, so the workgroups that share an L2 take one contiguous run
    const int b = (int)blockIdx.x;
    const int t = (b & 7) * (int)(gridDim.x >> 3) + (b >> 3);
    if (t >= a.ntiles) return;
    const int cb = t % a.ncb, xb = (t / a.ncb) % a.nxw, yb = t / (a.ncb * a.nxw);
    const int c0 = a.c_begin + cb * HP_CB, x0 = xb * HP_XW, y0 = yb * a.rs;
    const int y1 = min(y0 + a.rs, H);
    // alternate row direction by row block: the two tiles that share a halo row reach it at about the same time
    const int dir = (yb & 1) ? -1 : 1;
    if constexpr (WIN) {  // a tile without a marked texel: nothing read, nothing written
        int any = 0;
        for (int e = (int)threadIdx.x; e < (y1 - y0) * HP_XW; e += HP_NT) {
            const int yy = y0 + e / HP_XW, xx = x0 + e % HP_XW;
            any |= (xx < W && a.marks[(size_t)yy * W + xx]) ? 1 : 0;
        }
        if (!__syncthreads_or(any)) return;
    }
    if ((int)threadIdx.x < a.m.L) {
        const int l = (int)threadIdx.x;
        int first = 0;
        for (int j = 0; j < l; ++j) first += a.m.layer[j].C;
        const fmpnp_hc_layer &ly = a.m.layer[l];
        tab[l].data = ly.data;
        tab[l].stride_c = (size_t)ly.stride_c;
        tab[l].stride_y = (size_t)ly.stride_y;
        tab[l].sy = axis_scale(ly.H, H);
        tab[l].sx = axis_scale(ly.W, W);
        tab[l].H = ly.H;
        tab[l].W = ly.W;
        tab[l].first = first;
    }
    __syncthreads();
    HpUnits u;
    hp_units(u, a, tab, c0, x0);

    const int cc = (int)(threadIdx.x & 63u), c = c0 + cc;
    const int run = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int xr = x0 + run * HP_RUN, ncols = W - xr;
    const size_t tstride = (size_t)(GRAD ? 3 : 1) * (size_t)a.cs;
    Tout *const out = reinterpret_cast<Tout *>(a.out);
    const bool sn = a.sobel_normalized != 0;
    constexpr int AHEAD = GRAD ? 2 : 1;  // rows formed ahead of the one computed (f only: no halo rows)

    HpRow r;
    const int n = y1 - y0, ys = dir > 0 ? y0 : y1 - 1;
    if constexpr (GRAD) {
        hp_load(r, u, a, tab, x0, ys - dir);
        hp_store(r, u, a, tab, ys - dir, ring + ((ys - dir) & 3) * HP_SE);
    }
    hp_load(r, u, a, tab, x0, ys);
    hp_store(r, u, a, tab, ys, ring + (ys & 3) * HP_SE);
    if constexpr (GRAD) {
        hp_load(r, u, a, tab, x0, ys + dir);
        hp_store(r, u, a, tab, ys + dir, ring + ((ys + dir) & 3) * HP_SE);
    }
    for (int k = 0; k < n; ++k) {
        const int y = ys + k * dir;
        __syncthreads();  // the rows this one needs are in their slots; slot (y + AHEAD dir) & 3 is free
        const bool more = GRAD ? k + 2 <= n : k + 1 < n;
        if (more) hp_load(r, u, a, tab, x0, y + AHEAD * dir);
        if (c < a.c_end && ncols > 0) {
            const int lo = cc * HP_LD + run * HP_RUN;
            const float *rm = ring + ((y - 1) & 3) * HP_SE + lo;
            const float *r0 = ring + (y & 3) * HP_SE + lo;
            const float *rp = ring + ((y + 1) & 3) * HP_SE + lo;
            unsigned wm = 0;
            if constexpr (WIN) {  // the run's marks (wave-uniform bytes)
                const unsigned char *wr = a.marks + (size_t)y * W + xr;
#pragma unroll
                for (int j = 0; j < HP_RUN; ++j) wm |= (j < ncols && wr[j]) ? (1u << j) : 0u;
            }
            if (!WIN || wm)
                hp_row<Tout, GRAD, WIN>(rm, r0, rp, out + ((size_t)y * W + xr) * tstride + c, tstride, a.cs, ncols, wm,
                                        sn);
        }
        if (more) hp_store(r, u, a, tab, y + AHEAD * dir, ring + ((y + AHEAD * dir) & 3) * HP_SE);
    }
}

void fill_layers(HpLayers &m, const fmpnp_hc_layer *layers, int L, int item, int H, int W, long long C) {
    for (int l = 0; l < L; ++l) {
        m.layer[l] = layers[l];
        m.layer[l].data = layers[l].data + (size_t)item * (size_t)layers[l].stride_b;
    }
    m.L = L;
    m.H = H;
    m.W = W;
    m.C = (int)C;
}

}  // namespace

size_t hc_pack_workspace_bytes(int H, int W) { return align256((size_t)H * (size_t)W * sizeof(float)); }

int launch_hc_norm(const fmpnp_hc_layer *layers, int L, int item, int H, int W, long long C, float *norm,
                   const unsigned char *marks, hipStream_t s) {
    HnArgs a = {};
    fill_layers(a.m, layers, L, item, H, W, C);
    a.norm = norm;
    a.marks = marks;
    a.nblocks = (int)((C + BLOCK - 1) / BLOCK);
    a.tiles_x = (unsigned)((W + 63) / 64);
    const unsigned long long n_tiles = (unsigned long long)H * a.tiles_x;
    if (n_tiles > 0x7fffffffull - 8) return FMPNP_ETOOBIG;
    hipLaunchKernelGGL(hc_norm_kernel, dim3((unsigned)n_tiles), dim3(HN_NT), 0, s, a);
    return (int)hipGetLastError();
}

int launch_hc_pack(const fmpnp_hc_layer *layers, int L, int item, int H, int W, long long C, int c_begin, int c_end,
                   int layout, int dtype_out, int cs, int sobel_normalized, int replicate, const unsigned char *marks,
                   const float *norm, void *out, hipStream_t s) {
    HpArgs a = {};
    fill_layers(a.m, layers, L, item, H, W, C);
    a.norm = norm;
    a.marks = marks;
    a.out = out;
    a.c_begin = c_begin;
    a.c_end = c_end;
    a.cs = cs;
    a.replicate = replicate ? 1 : 0;
    a.sobel_normalized = sobel_normalized ? 1 : 0;
    // rows per workgroup as the Sobel pack's: about one resident wave of workgroups (4 per CU), >= 4 rows
    a.ncb = (c_end - c_begin + HP_CB - 1) / HP_CB;
    a.nxw = (W + HP_XW - 1) / HP_XW;
    long long nyb = 1024 / ((long long)a.ncb * a.nxw);
    if (nyb < 1) nyb = 1;
    long long rs = (H + nyb - 1) / nyb;
    if (rs < 4) rs = 4;
    nyb = (H + rs - 1) / rs;
    const long long ntiles = (long long)a.ncb * a.nxw * nyb;
    if (ntiles > 0x7fffffffll - 8) return FMPNP_ETOOBIG;
    a.rs = (int)rs;
    a.ntiles = (int)ntiles;
    const dim3 grid((unsigned)((ntiles + 7) / 8 * 8)), block(HP_NT);
    const bool grad = layout == FMPNP_LAYOUT_FGRAD;
    if (!grad) {
        if (marks) hipLaunchKernelGGL((hc_pack_kernel<float, false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hc_pack_kernel<float, false, false>), grid, block, 0, s, a);
    } else if (dtype_out == FMPNP_F64) {
        if (marks) hipLaunchKernelGGL((hc_pack_kernel<double, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hc_pack_kernel<double, true, false>), grid, block, 0, s, a);
    } else {
        if (marks) hipLaunchKernelGGL((hc_pack_kernel<float, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hc_pack_kernel<float, true, false>), grid, block, 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace fmpnp
