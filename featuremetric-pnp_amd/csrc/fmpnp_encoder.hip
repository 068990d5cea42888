// fmpnp_encoder.hip -- the encoder's operators on gfx950 (include/fmpnp.h, "the encoder's operators"): what
// VGG-16's features[:-2] (s2dhm/network/network.py:47-51) is made of.
//
//   conv3x3_kernel      3x3 / stride 1 convolution of dilation and padding D (1; 2 for fmpnp_conv3x3_dilated) as an
//                       implicit GEMM on v_mfma_f32_32x32x2_f32:
//                       out[co][pixel] = sum_k w[co][k] * tap_k(pixel), k = ci * 9 + ky * 3 + kx.  Every output is
//                       one accumulator's fmaf chain over k ascending from +0 (the MFMA is that chain bit for bit,
//                       corr_kernel of fmpnp_match.hip), the taps outside the image and the zero-padded k tail add
//                       fma(0, w, acc): no split-K, no atomics, so a value does not depend on the tile or the
//                       grid.  The weights are the [Cout][9 Cin] operand as they lie in memory; the tap operand is
//                       never formed: a block stages the input halo of its pixel tile in LDS and the MFMA's lanes
//                       read it at tap-shifted addresses.  Bias, ReLU and the store are the epilogue.
//   relu_kernel         x > 0 ? x : (x != x ? x : +0), streaming, 16-byte accesses where the pointers allow.
//   maxpool2x2_kernel   2x2 / stride 2 / floor: two 16-byte row reads and one 8-byte store per thread where the
//                       rows allow, one output per thread otherwise.
//
// The same expressions run on the host in fmpnp_encoder_cpu.cpp (the twins).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- convolution --------------------------------------------------------------------------------
// A workgroup of 4 waves forms BM output channels x BN pixels, each wave 2 x 2 tiles of 32 x 32: 128 x 128 with
// the waves 2 x 2 (corr_kernel's decomposition), or, for layers of at most 64 output channels (VGG-16's first
// block), 64 x 256 with the four waves side by side along the pixels, so that no wave's rows are padding.  k
// advances KC input channels = BK = 36 taps at a time (18 MFMA steps of 2).  Which form runs changes no value.
// The pixel tile is TR rows x TW columns of the image, TW = 1 << lw in 4 .. BN and TR = BN / TW: BN consecutive
// x of one row for a wide image, several short rows when W is below BN.  Pixel n of the tile is
// (n >> lw, n & (TW - 1)).
// The dilation D (1, or 2 for fmpnp_conv3x3_dilated: padding D, tap (ky, kx) at ((ky - 1) D, (kx - 1) D)) is a
// compile-time constant: the halo grows to (TR + 2 D) x (TW + 2 D) and the taps step D texels in it; the chain,
// the weight tile and the epilogue do not know it.  At D = 2 a one-row tile would stage five halo rows per output
// row, so its widest tile is the shorter, taller TW = 1 << FMPNP_CONV_D2_LW (DESIGN.md 4.16 has the table the
// choice was kept by; the choice changes no value).
#ifndef FMPNP_CONV_D2_LW
#define FMPNP_CONV_D2_LW 5
#endif
constexpr int KC = 4, BK = 9 * KC, CONV_NT = 256;
// (TR + 2 D)(TW + 2 D) at its largest over the tile forms TW = 1 << lw, lw = 2 .. lw_max
constexpr int halo_max(int BN, int D, int lw_max) {
    int m = 0;
    for (int lw = 2; lw <= lw_max; ++lw) {
        const int h = ((BN >> lw) + 2 * D) * ((1 << lw) + 2 * D);
        m = h > m ? h : m;
    }
    return m;
}
// LDS images.  Ws[k][m], k-major (the weight tile transposed; the odd row stride spreads the transposed writes
// over the banks).  Hs[ci][hy][hx]: the halo, (TR + 2 D) x (TW + 2 D) per channel; at D = 1 at most 3 x (BN + 2).
template <int MW, int D>  // waves along the output channels: 2 or 1; the dilation: 1 or 2
struct ConvTile {
    static constexpr int BM = 64 * MW, BN = 64 * (4 / MW);
    static constexpr int LW_FULL = BN == 128 ? 7 : 8;                 // TW = BN: a one-row tile
    static constexpr int LW_MAX = D == 1 ? LW_FULL : (FMPNP_CONV_D2_LW < LW_FULL ? FMPNP_CONV_D2_LW : LW_FULL);
    static constexpr int WS_LD = BM + 1;
    static constexpr int HALO_MAX = halo_max(BN, D, LW_MAX);          // D = 1: 3 (BN + 2), the one-row tile's
    static constexpr int W_PER_T = BM * BK / CONV_NT;                 // 18 or 9
    static constexpr int H_PER_T = (KC * HALO_MAX + CONV_NT - 1) / CONV_NT;  // D = 1: 7 or 13
    static_assert(MW == 1 || MW == 2, "four waves: 2 x 2 or 1 x 4");
    static_assert(D == 1 || D == 2, "the dilations built");
    static_assert(LW_MAX >= 2, "TW = 4 at least");
    static_assert(D != 1 || HALO_MAX == 3 * (BN + 2), "the D = 1 halo is what it was");
    static_assert(BM * BK % CONV_NT == 0 && BK % 2 == 0, "the weight tile deals out evenly; k in MFMA steps of 2");
};

template <int MW, int D>
__global__ __launch_bounds__(CONV_NT) void conv3x3_kernel(const float *__restrict__ in, int Cin, int H, int W,
                                                          const float *__restrict__ weight,
                                                          const float *__restrict__ bias, int Cout, int flags,
                                                          float *__restrict__ out, int lw, int tiles_x, int ptiles,
                                                          int ctiles) {
    using T = ConvTile<MW, D>;
    constexpr int BM = T::BM, BN = T::BN, WS_LD = T::WS_LD, HALO_MAX = T::HALO_MAX, W_PER_T = T::W_PER_T,
                  H_PER_T = T::H_PER_T;
    __shared__ float Ws[BK * WS_LD];
    __shared__ float Hs[KC * HALO_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block -> (pixel tile, channel tile, image): pixel tiles fastest, so the blocks in flight share one weight tile
    int id = blockIdx.x;
    const int pt = id % ptiles;
    id /= ptiles;
    const int ct = id % ctiles, b = id / ctiles;
    const int TW = 1 << lw, TR = BN >> lw, RS = TW + 2 * D, CS = (TR + 2 * D) * RS;  // halo row and channel strides
    const int y0 = (pt / tiles_x) * TR, x0 = (pt % tiles_x) * TW, co0 = ct * BM;
    const int K = 9 * Cin, HW = H * W;  // (every tensor is below 2^31 elements: 32-bit offsets within one)
    const float *img = in + (size_t)b * Cin * HW;

    // global -> register staging.  Weight element e of this thread is flat index e * 256 + tid of the [BM][36]
    // tile: (m, k) = (idx / 36, idx % 36), 36 consecutive floats of a weight row per m.  Halo element e is flat
    // index e * 256 + tid of [KC][TR + 2 D][TW + 2 D]; its place in the image does not change from k tile to k tile,
    // so the offsets are formed once: hoff = ci * HW + y * W + x, or -1 outside the image (or past the halo, or for
    // a channel no k tile has).
    int hoff[H_PER_T], hci[H_PER_T];
#pragma unroll
    for (int e = 0; e < H_PER_T; ++e) {
        const int idx = e * CONV_NT + tid;
        const int ci = idx / CS, rem = idx - ci * CS, hy = rem / RS, hx = rem - hy * RS;
        const int y = y0 + hy - D, x = x0 + hx - D;
        const bool inside = ci < KC && ci < Cin && y >= 0 && y < H && x >= 0 && x < W;
        hci[e] = ci;
        hoff[e] = inside ? ci * HW + y * W + x : -1;
    }
    float rw[W_PER_T], rh[H_PER_T];
    auto fetch = [&](int c0) {  // the k tile of input channels c0 .. c0 + KC - 1
#pragma unroll
        for (int e = 0; e < W_PER_T; ++e) {
            const int idx = e * CONV_NT + tid, m = idx / BK, k = c0 * 9 + (idx - m * BK);
            rw[e] = (co0 + m < Cout && k < K) ? weight[(size_t)(co0 + m) * K + k] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < H_PER_T; ++e)
            rh[e] = (hoff[e] >= 0 && c0 + hci[e] < Cin) ? img[(size_t)c0 * HW + hoff[e]] : 0.f;
    };
    // The MFMA's lanes: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31].  Step s of a k tile holds
    // taps k = 2 s + h of the tile; a lane's halo offset for it is the tap's (ci, ky, kx) in the halo's strides,
    // the same for every k tile, plus the lane's pixel.
    const int r = lane & 31, h = lane >> 5;
    const int wm = MW == 2 ? (wave >> 1) * 64 : 0, wn = MW == 2 ? (wave & 1) * 64 : wave * 64;
    int tap[BK / 2];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
        const int k = 2 * s + h, ci = k / 9, t = k - ci * 9, ky = t / 3, kx = t - ky * 3;
        tap[s] = ci * CS + ky * D * RS + kx * D;
    }
    int pix[2];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int n = wn + bb * 32 + r;
        pix[bb] = (n >> lw) * RS + (n & (TW - 1));  // halo (ty + ky D, tx + kx D) is the tap (ky - 1, kx - 1) of the pixel
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][bb][g] = 0.f;
    fetch(0);
    for (int c0 = 0; c0 < Cin; c0 += KC) {
        __syncthreads();  // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < W_PER_T; ++e) {
            const int idx = e * CONV_NT + tid, m = idx / BK, k = idx - m * BK;
            Ws[k * WS_LD + m] = rw[e];
        }
#pragma unroll
        for (int e = 0; e < H_PER_T; ++e) {
            const int idx = e * CONV_NT + tid;
            if (idx < KC * CS) Hs[idx] = rh[e];
        }
        __syncthreads();
        if (c0 + KC < Cin) fetch(c0 + KC);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const float a0 = Ws[(2 * s + h) * WS_LD + wm + r], a1 = Ws[(2 * s + h) * WS_LD + wm + 32 + r];
            const float b0 = Hs[tap[s] + pix[0]], b1 = Hs[tap[s] + pix[1]];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  The
    // column is the pixel: a wave's lanes store consecutive x.
    const bool has_bias = (flags & FMPNP_CONV_BIAS) != 0, do_relu = (flags & FMPNP_CONV_RELU) != 0;
    float *dst = out + (size_t)b * Cout * HW;
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int n = wn + bb * 32 + r, y = y0 + (n >> lw), x = x0 + (n & (TW - 1));
        if (y >= H || x >= W) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int co = co0 + wm + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
                if (co < Cout)
                    dst[(size_t)co * HW + y * W + x] = enc::finish(acc[a][bb][g], has_bias, has_bias ? bias[co] : 0.f, do_relu);
            }
    }
}

// ---- ReLU and max-pool --------------------------------------------------------------------------
constexpr int STREAM_NT = 256;

__global__ __launch_bounds__(STREAM_NT) void relu_kernel(const float *in, float *out, long long n, int vec) {
    const long long i = (long long)blockIdx.x * STREAM_NT + threadIdx.x;
    if (vec) {  // n / 4 whole float4 (both pointers 16-byte aligned), then the tail
        if (i < n / 4) {
            float4 v = ((const float4 *)in)[i];
            v.x = enc::relu(v.x), v.y = enc::relu(v.y), v.z = enc::relu(v.z), v.w = enc::relu(v.w);
            ((float4 *)out)[i] = v;
        }
        const long long t = n / 4 * 4 + i;
        if (i < 4 && t < n) out[t] = enc::relu(in[t]);
    } else if (i < n) {
        out[i] = enc::relu(in[i]);
    }
}
// (in and out may be one buffer: every element is read by the thread that writes it, before it writes)

// vec: W % 4 == 0 and the pointers aligned, so a thread's float4 of each of the two rows holds two whole windows
__global__ __launch_bounds__(STREAM_NT) void maxpool2x2_kernel(const float *__restrict__ in, int H, int W,
                                                               float *__restrict__ out, long long n_out, int vec) {
    const int OH = H / 2, OW = W / 2;
    const long long i = (long long)blockIdx.x * STREAM_NT + threadIdx.x;
    if (vec) {
        if (i >= n_out / 2) return;
        const int pw = OW / 2;  // pairs per output row
        const long long row = i / pw;
        const int px = (int)(i - row * pw), oy = (int)(row % OH);
        const long long plane = row / OH;
        const float *r0 = in + ((size_t)plane * H + 2 * oy) * W + 4 * px;
        const float4 u = *(const float4 *)r0, l = *(const float4 *)(r0 + W);
        float2 o;
        o.x = enc::pool4(u.x, u.y, l.x, l.y);
        o.y = enc::pool4(u.z, u.w, l.z, l.w);
        *(float2 *)(out + (size_t)row * OW + 2 * px) = o;
    } else {
        if (i >= n_out) return;
        const long long row = i / OW;
        const int ox = (int)(i - row * OW), oy = (int)(row % OH);
        const long long plane = row / OH;
        const float *r0 = in + ((size_t)plane * H + 2 * oy) * W + 2 * ox;
        out[i] = enc::pool4(r0[0], r0[1], r0[W], r0[W + 1]);
    }
}

}  // namespace

}  // namespace fmpnp

using namespace fmpnp;

namespace {

// validated arguments -> one launch of the <MW> form; 0, FMPNP_ETOOBIG or a hipError_t
template <int MW, int D>
int launch_conv(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout, int flags,
                float *out, hipStream_t s) {
    using T = ConvTile<MW, D>;
    int lw = 2;  // TW = 4 at least; the smallest power of two that holds a row, 1 << LW_MAX at most (D = 1: BN)
    while (lw < T::LW_MAX && (1 << lw) < W) ++lw;
    const int TW = 1 << lw, TR = T::BN >> lw;
    const size_t tiles_x = ((size_t)W + TW - 1) / TW, tiles_y = ((size_t)H + TR - 1) / TR;
    const size_t ptiles = tiles_x * tiles_y, ctiles = ((size_t)Cout + T::BM - 1) / T::BM;
    if (ptiles > (size_t)INT32_MAX || ptiles * ctiles > (size_t)INT32_MAX || ptiles * ctiles * (size_t)B > (size_t)INT32_MAX)
        return FMPNP_ETOOBIG;
    hipLaunchKernelGGL((conv3x3_kernel<MW, D>), dim3((unsigned)(ptiles * ctiles * (size_t)B)), dim3(CONV_NT), 0, s, in, Cin, H,
                       W, weight, bias, Cout, flags, out, lw, (int)tiles_x, (int)ptiles, (int)ctiles);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int fmpnp_conv3x3_async(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                        int flags, float *out, void *hip_stream) {
    const int rc = enc::conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out);
    if (rc) return rc;
    return Cout <= 64 ? launch_conv<1, 1>(in, B, Cin, H, W, weight, bias, Cout, flags, out, (hipStream_t)hip_stream)
                      : launch_conv<2, 1>(in, B, Cin, H, W, weight, bias, Cout, flags, out, (hipStream_t)hip_stream);
}

// (dilation 1 is fmpnp_conv3x3_async's own launch)
int fmpnp_conv3x3_dilated_async(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                                int Cout, int flags, float *out, int dilation, void *hip_stream) {
    const int rc = enc::conv_dilated_args(in, B, Cin, H, W, weight, bias, Cout, flags, out, dilation);
    if (rc) return rc;
    if (dilation == 1) return fmpnp_conv3x3_async(in, B, Cin, H, W, weight, bias, Cout, flags, out, hip_stream);
    return Cout <= 64 ? launch_conv<1, 2>(in, B, Cin, H, W, weight, bias, Cout, flags, out, (hipStream_t)hip_stream)
                      : launch_conv<2, 2>(in, B, Cin, H, W, weight, bias, Cout, flags, out, (hipStream_t)hip_stream);
}

int fmpnp_conv3x3_dilated(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                          int flags, float *out, int dilation, void *hip_stream) {
    const int rc = fmpnp_conv3x3_dilated_async(in, B, Cin, H, W, weight, bias, Cout, flags, out, dilation, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

int fmpnp_conv3x3(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout, int flags,
                  float *out, void *hip_stream) {
    const int rc = fmpnp_conv3x3_async(in, B, Cin, H, W, weight, bias, Cout, flags, out, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

int fmpnp_relu_async(const float *in, float *out, long long n, void *hip_stream) {
    const int rc = enc::relu_args(in, out, n);
    if (rc) return rc;
    if (n == 0) return 0;
    const int vec = n >= 4 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const long long threads = vec ? (n / 4 > 4 ? n / 4 : 4) : n;
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((threads + STREAM_NT - 1) / STREAM_NT)), dim3(STREAM_NT), 0,
                       (hipStream_t)hip_stream, in, out, n, vec);
    return (int)hipGetLastError();
}

int fmpnp_maxpool2x2_async(const float *in, int B, int C, int H, int W, float *out, void *hip_stream) {
    const int rc = enc::pool_args(in, B, C, H, W, out);
    if (rc) return rc;
    const long long n_out = (long long)B * C * (H / 2) * (W / 2);
    const int vec = W % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0;
    const long long threads = vec ? n_out / 2 : n_out;
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)((threads + STREAM_NT - 1) / STREAM_NT)), dim3(STREAM_NT), 0,
                       (hipStream_t)hip_stream, in, H, W, out, n_out, vec);
    return (int)hipGetLastError();
}

int fmpnp_maxpool2x2(const float *in, int B, int C, int H, int W, float *out, void *hip_stream) {
    const int rc = fmpnp_maxpool2x2_async(in, B, C, H, W, out, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

}  // extern "C"
