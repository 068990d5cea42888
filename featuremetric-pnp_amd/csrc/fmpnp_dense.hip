// fmpnp_dense.hip -- the two operators a D2-Net style dense-feature walk needs beside the encoder's (include/fmpnp.h,
// "dense features"): VGG-16 to conv4_3 with pool3 an AvgPool2d(2, stride 1) and conv4 dilated by 2 (the dilated
// convolution is conv3x3_kernel<MW, 2> of fmpnp_encoder.hip), and the scale pyramid of
// s2dhm/d2net_utils/dense_pyramid.py:5-42.
//
//   avgpool2x2s1_kernel   2x2 / stride 1 / no padding: out [B][C][H - 1][W - 1], one output per thread, enc::avg4.
//   pyramid_step_kernel   out = normalise(cur + resize(prev)): the assembly's bilinear resize (align_corners=True),
//                         one fp32 add, and the assembly's norm -- fp64 chains per 64-channel block, the blocks
//                         combined in block order -- with F.normalize's clamp.  One workgroup of 8 waves owns 64
//                         consecutive texels of one output row, as hypercolumn_kernel does: pass 1 deals the blocks
//                         over the waves and every wave ends with the same n per texel, pass 2 recomputes the values
//                         of a wave's eighth of the channels with the same code and stores v / max(n, 1e-12f).  cur
//                         and prev are read twice through the caches; out is written once.  out may be cur: a
//                         texel's channels are read (both passes) and written by one workgroup, the last barrier of
//                         pass 1 lies between its last pass-1 read and its first store, and pass 2 reads an element
//                         in the thread that then writes it.
//
// Built with -ffp-contract=off; every value is formed by the functions of the *_impl.h headers, which the CPU twins
// (fmpnp_dense_cpu.cpp) call too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_dense_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {
namespace {

constexpr int STREAM_NT = 256;

__global__ __launch_bounds__(STREAM_NT) void avgpool2x2s1_kernel(const float *__restrict__ in, int H, int W,
                                                                 float *__restrict__ out, long long n_out) {
    const int OH = H - 1, OW = W - 1;
    const long long i = (long long)blockIdx.x * STREAM_NT + threadIdx.x;
    if (i >= n_out) return;
    const long long row = i / OW;
    const int ox = (int)(i - row * OW), oy = (int)(row % OH);
    const long long plane = row / OH;
    const float *r0 = in + ((size_t)plane * H + oy) * W + ox;  // (oy + 1 <= H - 1 and ox + 1 <= W - 1)
    out[i] = enc::avg4(r0[0], r0[1], r0[W], r0[W + 1]);
}

using namespace hc;

constexpr int PY_NW = 8, PY_NT = 64 * PY_NW;

struct PyrArgs {
    const float *cur, *prev;  // (no __restrict__: out may be cur)
    float *out;
    int C, h, w, hp, wp, nblocks;
    unsigned tiles_x;
};

template <bool PREV, bool NORM>
__global__ __launch_bounds__(PY_NT) void pyramid_step_kernel(const PyrArgs a) {
    __shared__ double part[2][PY_NW][64];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned row = blockIdx.x / a.tiles_x;
    const int y = (int)(row % (unsigned)a.h), b = (int)(row / (unsigned)a.h);
    const int x = (int)(blockIdx.x % a.tiles_x) * 64 + lane;
    const int xr = min(x, a.w - 1);  // (a lane past the row's end reads its last texel and stores nothing)

    const size_t cs = (size_t)a.h * (size_t)a.w, ps = PREV ? (size_t)a.hp * (size_t)a.wp : 0;
    const size_t cur0 = ((size_t)b * (size_t)a.C * (size_t)a.h + (size_t)y) * (size_t)a.w + (size_t)xr;
    Tap ty = {}, tx = {};
    const float *p0 = nullptr, *p1 = nullptr;
    if (PREV) {
        ty = axis_tap(axis_scale(a.hp, a.h), a.hp, y);
        tx = axis_tap(axis_scale(a.wp, a.w), a.wp, xr);
        const float *pb = a.prev + (size_t)b * (size_t)a.C * ps;
        p0 = pb + (size_t)ty.i0 * (size_t)a.wp;
        p1 = pb + (size_t)ty.i1 * (size_t)a.wp;
    }
    auto value = [&](int c) {
        float v = a.cur[cur0 + (size_t)c * cs];
        if (PREV) {
            const float *q0 = p0 + (size_t)c * ps, *q1 = p1 + (size_t)c * ps;
            v = dense::summed(v, bilerp(q0[tx.i0], q0[tx.i1], q1[tx.i0], q1[tx.i1], tx.w0, tx.w1, ty.w0, ty.w1));
        }
        return v;
    };
    // body(c, v) for c in [c_begin, c_end) ascending; the values of four channels are formed before any is used,
    // so their loads are in flight together
    auto walk = [&](int c_begin, int c_end, auto &&body) {
        int c = c_begin;
        for (; c + 4 <= c_end; c += 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = value(c + u);
#pragma unroll
            for (int u = 0; u < 4; ++u) body(c + u, v[u]);
        }
        for (; c < c_end; ++c) body(c, value(c));
    };

    float dv = 1.0f;
    if (NORM) {
        double sum = 0.0;
        for (int r0 = 0, r = 0; r0 < a.nblocks; r0 += PY_NW, ++r) {
            const int blk = r0 + wave;
            double acc = 0.0;
            if (blk < a.nblocks)
                walk(blk * BLOCK, min(a.C, blk * BLOCK + BLOCK), [&](int, float v) { acc = square_acc(v, acc); });
            // two buffers, one barrier per round: a wave writes round r + 2's partials only after the barrier of
            // round r + 1, which every wave reaches after it has read round r's
            double(*p)[64] = part[r & 1];
            p[wave][lane] = acc;
            __syncthreads();
            const int nb = min(PY_NW, a.nblocks - r0);
            for (int j = 0; j < nb; ++j) sum = sum + p[j][lane];
        }
        dv = dense::divisor(norm_of(sum));
    }

    const int c0 = (int)((long long)a.C * wave / PY_NW), c1 = (int)((long long)a.C * (wave + 1) / PY_NW);
    const bool inside = x < a.w;
    walk(c0, c1, [&](int c, float v) {
        if (inside) a.out[cur0 + (size_t)c * cs] = NORM ? normalised(v, dv) : v;
    });
}

}  // namespace
}  // namespace fmpnp

using namespace fmpnp;

extern "C" {

int fmpnp_avgpool2x2s1_async(const float *in, int B, int C, int H, int W, float *out, void *hip_stream) {
    const int rc = enc::pool_args(in, B, C, H, W, out);
    if (rc) return rc;
    const long long n_out = (long long)B * C * (H - 1) * (W - 1);  // (below the input's 2^31)
    hipLaunchKernelGGL(avgpool2x2s1_kernel, dim3((unsigned)((n_out + STREAM_NT - 1) / STREAM_NT)), dim3(STREAM_NT), 0,
                       (hipStream_t)hip_stream, in, H, W, out, n_out);
    return (int)hipGetLastError();
}

int fmpnp_avgpool2x2s1(const float *in, int B, int C, int H, int W, float *out, void *hip_stream) {
    const int rc = fmpnp_avgpool2x2s1_async(in, B, C, H, W, out, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

int fmpnp_dense_pyramid_step_async(const float *cur, const float *prev, int B, int C, int h, int w, int hp, int wp,
                                   float *out, int flags, void *hip_stream) {
    const int rc = dense::step_args(cur, prev, B, C, h, w, hp, wp, out, flags);
    if (rc) return rc;
    PyrArgs a = {};
    a.cur = cur;
    a.prev = prev;
    a.out = out;
    a.C = C;
    a.h = h;
    a.w = w;
    a.hp = prev ? hp : 1;
    a.wp = prev ? wp : 1;
    a.nblocks = (C + hc::BLOCK - 1) / hc::BLOCK;
    a.tiles_x = (unsigned)((w + 63) / 64);
    // (B h ceil(w / 64) <= B C h w < 2^31)
    const dim3 grid((unsigned)((size_t)B * (size_t)h * a.tiles_x)), block(PY_NT);
    const hipStream_t s = (hipStream_t)hip_stream;
    const bool norm = (flags & FMPNP_PYR_NORMALIZE) != 0;
    if (prev) {
        if (norm) hipLaunchKernelGGL((pyramid_step_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((pyramid_step_kernel<true, false>), grid, block, 0, s, a);
    } else {
        if (norm) hipLaunchKernelGGL((pyramid_step_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((pyramid_step_kernel<false, false>), grid, block, 0, s, a);
    }
    return (int)hipGetLastError();
}

int fmpnp_dense_pyramid_step(const float *cur, const float *prev, int B, int C, int h, int w, int hp, int wp, float *out,
                             int flags, void *hip_stream) {
    const int rc = fmpnp_dense_pyramid_step_async(cur, prev, B, C, h, w, hp, wp, out, flags, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

}  // extern "C"
