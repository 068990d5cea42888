// fmpnp_hypercolumn.hip -- the hypercolumn assembly kernel (s2dhm/network/network.py:149-173): bilinear
// resize of every layer (align_corners=True), channel concatenation and the per-texel L2 normalisation
// in one launch.  include/fmpnp.h states the numeric contract; every value is formed by the functions of
// fmpnp_hypercolumn_impl.h, which the CPU twin calls too.  Built with -ffp-contract=off.
//
// One workgroup of 8 waves owns one tile of 64 * VEC consecutive texels of one output row (lane i: texels
// VEC i .. VEC i + VEC - 1, so a wave's store instruction covers one contiguous line; VEC = 1, 4-byte
// stores of 256-byte lines, is the launch's choice because it measured faster; VEC = 4, 16-byte stores
// where the output's alignment allows them, on request).  The channels are dealt over the waves:
//   pass 1: wave w forms the fp64 partials of the 64-channel blocks w, w + 8, ...; after each round of 8
//           blocks the partials meet in LDS and every wave adds them to its own copy of the running sum in
//           ascending block order, so every wave ends with the same n = (float)sqrt(sum) per texel;
//   pass 2: wave w recomputes the values of its eighth of the channels with the same code and stores v / n.
// The taps and weights depend on (layer, texel) only: they are set up once per layer segment, outside the
// channel loop.  The layers are read twice through the caches; the output is written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_hypercolumn_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {
namespace {

using namespace hc;

constexpr int HC_NW = 8, HC_NT = 64 * HC_NW;

struct HcArgs {
    fmpnp_hc_layer layer[MAX_LAYERS];
    float *out;
    size_t osb, osc, osy;
    int L, H, W, C, nblocks;
    // the tiles (batch item, row, tile along x) in row-major order; workgroup g takes tile
    // (g % 8) * tiles_per_group + g / 8: the workgroups that share an L2 (g % 8 labels them) take
    // neighbouring rows, which read the same rows of the layers
    unsigned tiles_x, n_tiles, tiles_per_group;
};

// one layer's taps for this lane's texels of row y
template <int VEC>
struct Geo {
    const float *r0, *r1;  // rows y0 and y1 of the batch item's channel 0 (the same in every lane)
    size_t cs;
    unsigned x0[VEC], x1[VEC];  // byte offsets in a row (32 bits; the row's base is the same in every lane)
    float w0x[VEC], w1x[VEC], w0y, w1y;
};

template <int VEC>
__device__ inline void set_layer(Geo<VEC> &g, const fmpnp_hc_layer &ly, int b, int y, int x, int H, int W) {
    const Tap ty = axis_tap(axis_scale(ly.H, H), ly.H, y);
    const float *base = ly.data + (size_t)b * (size_t)ly.stride_b;
    g.r0 = base + (size_t)ty.i0 * (size_t)ly.stride_y;
    g.r1 = base + (size_t)ty.i1 * (size_t)ly.stride_y;
    g.cs = (size_t)ly.stride_c;
    g.w0y = ty.w0;
    g.w1y = ty.w1;
    const float sx = axis_scale(ly.W, W);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const Tap tx = axis_tap(sx, ly.W, min(x + k, W - 1));  // (a lane past the row's end reads its last texel)
        g.x0[k] = 4u * (unsigned)tx.i0;
        g.x1[k] = 4u * (unsigned)tx.i1;
        g.w0x[k] = tx.w0;
        g.w1x[k] = tx.w1;
    }
}

__device__ inline float at(const float *row, unsigned byte_offset) {
    return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(row) + byte_offset);
}

// body(c, v): the resized values v[VEC] of concatenated channel c, for c in [c_begin, c_end) ascending
template <int VEC, class F>
__device__ inline void walk(const HcArgs &a, int b, int y, int x, int c_begin, int c_end, F &&body) {
    int first = 0;  // the layer's first concatenated channel
    for (int l = 0; l < a.L && first < c_end; ++l) {
        const fmpnp_hc_layer &ly = a.layer[l];
        const int lo = max(c_begin, first), hi = min(c_end, first + ly.C);
        if (lo < hi) {
            Geo<VEC> g;
            set_layer(g, ly, b, y, x, a.H, a.W);
            const float *p0 = g.r0 + (size_t)(lo - first) * g.cs, *p1 = g.r1 + (size_t)(lo - first) * g.cs;
            // the taps of U channels are loaded before any is used: 32 independent loads in flight per lane
            constexpr int U = 8 / VEC;
            int c = lo;
            for (; c + U <= hi; c += U, p0 += U * g.cs, p1 += U * g.cs) {
                float t[U][VEC][4];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float *q0 = p0 + u * g.cs, *q1 = p1 + u * g.cs;
                        t[u][k][0] = at(q0, g.x0[k]);
                        t[u][k][1] = at(q0, g.x1[k]);
                        t[u][k][2] = at(q1, g.x0[k]);
                        t[u][k][3] = at(q1, g.x1[k]);
                    }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float v[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k)
                        v[k] = bilerp(t[u][k][0], t[u][k][1], t[u][k][2], t[u][k][3], g.w0x[k], g.w1x[k], g.w0y, g.w1y);
                    body(c + u, v);
                }
            }
            for (; c < hi; ++c, p0 += g.cs, p1 += g.cs) {
                float v[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    v[k] = bilerp(at(p0, g.x0[k]), at(p0, g.x1[k]), at(p1, g.x0[k]), at(p1, g.x1[k]), g.w0x[k], g.w1x[k],
                                  g.w0y, g.w1y);
                body(c, v);
            }
        }
        first += ly.C;
    }
}

template <int VEC, bool NORM>
__global__ __launch_bounds__(HC_NT) void hypercolumn_kernel(const HcArgs a) {
    constexpr int TILE = 64 * VEC;
    __shared__ double part[2][HC_NW][TILE];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned t = (blockIdx.x & 7u) * a.tiles_per_group + (blockIdx.x >> 3);
    if (t >= a.n_tiles) return;  // (the whole workgroup, before any barrier)
    const unsigned row = t / a.tiles_x;
    const int y = (int)(row % (unsigned)a.H), b = (int)(row / (unsigned)a.H);
    const int x = (int)(t % a.tiles_x) * TILE + lane * VEC;

    float n[VEC];
    if (NORM) {
        double sum[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) sum[k] = 0.0;
        for (int r0 = 0, r = 0; r0 < a.nblocks; r0 += HC_NW, ++r) {
            const int blk = r0 + wave;
            double acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.0;
            if (blk < a.nblocks)
                walk<VEC>(a, b, y, x, blk * BLOCK, min(a.C, blk * BLOCK + BLOCK), [&](int, const float(&v)[VEC]) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = square_acc(v[k], acc[k]);
                });
            // two buffers, one barrier per round: a wave writes round r + 2's partials only after the
            // barrier of round r + 1, which every wave reaches after it has read round r's
            double(*p)[TILE] = part[r & 1];
#pragma unroll
            for (int k = 0; k < VEC; ++k) p[wave][k * 64 + lane] = acc[k];
            __syncthreads();
            const int nb = min(HC_NW, a.nblocks - r0);
            for (int j = 0; j < nb; ++j)
#pragma unroll
                for (int k = 0; k < VEC; ++k) sum[k] = sum[k] + p[j][k * 64 + lane];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) n[k] = norm_of(sum[k]);
    }

    const int c0 = (int)((long long)a.C * wave / HC_NW), c1 = (int)((long long)a.C * (wave + 1) / HC_NW);
    float *orow = a.out + (size_t)b * a.osb + (size_t)y * a.osy;
    const bool inside = x < a.W;  // (VEC = 4: W is a multiple of 4, so a lane's texels are all inside or all outside)
    walk<VEC>(a, b, y, x, c0, c1, [&](int c, const float(&v)[VEC]) {
        float *o = orow + (size_t)c * a.osc;
        float q[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) q[k] = NORM ? normalised(v[k], n[k]) : v[k];
        if (inside) {
            if constexpr (VEC == 4)
                *reinterpret_cast<float4 *>(o + x) = make_float4(q[0], q[1], q[2], q[3]);
            else
                o[x] = q[0];
        }
    });
}

}  // namespace

int launch_hypercolumn(const fmpnp_hc_layer *layers, int L, int B, float *out, int H, int W, long long osb,
                       long long osc, long long osy, long long C, int flags, hipStream_t s) {
    HcArgs a = {};
    for (int l = 0; l < L; ++l) a.layer[l] = layers[l];
    a.out = out;
    a.osb = (size_t)osb;
    a.osc = (size_t)osc;
    a.osy = (size_t)osy;
    a.L = L;
    a.H = H;
    a.W = W;
    a.C = (int)C;
    a.nblocks = (int)((C + BLOCK - 1) / BLOCK);
    // 16-byte stores need every (b, c, y, 4 i) of the output on a 16-byte boundary.  Left to the library, the
    // stores are the 4-byte ones: a wave then writes one contiguous 256-byte line per instruction and four times
    // as many workgroups fill the device, which measured faster at every shape tried
    const bool aligned = W % 4 == 0 && ((uintptr_t)out & 15) == 0 && osb % 4 == 0 && osc % 4 == 0 && osy % 4 == 0;
    const bool vec4 = aligned && (flags & FMPNP_HC_VECTOR_STORES) && !(flags & FMPNP_HC_DWORD_STORES);
    const int tile = vec4 ? 256 : 64;
    a.tiles_x = (unsigned)((W + tile - 1) / tile);
    const unsigned long long n_tiles = (unsigned long long)B * (unsigned long long)H * a.tiles_x;
    if (n_tiles > 0x7fffffffull - 8) return FMPNP_ETOOBIG;
    a.n_tiles = (unsigned)n_tiles;
    a.tiles_per_group = (a.n_tiles + 7) / 8;
    const dim3 grid(8 * a.tiles_per_group), block(HC_NT);
    const bool norm = (flags & FMPNP_HC_NORMALIZE) != 0;
    if (vec4) {
        if (norm) hipLaunchKernelGGL((hypercolumn_kernel<4, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hypercolumn_kernel<4, false>), grid, block, 0, s, a);
    } else {
        if (norm) hipLaunchKernelGGL((hypercolumn_kernel<1, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((hypercolumn_kernel<1, false>), grid, block, 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace fmpnp
