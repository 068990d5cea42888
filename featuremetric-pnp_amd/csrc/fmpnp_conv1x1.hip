// fmpnp_conv1x1.hip -- the 1x1 / stride 1 / padding 0 convolution on gfx950 (include/fmpnp.h, "the 1x1
// convolution"): SuperPoint's two head convolutions, convPb (256 -> 65) and convDb (256 -> 256).
//
//   conv1x1_kernel      out[b][co][p] = sum_ci w[co][ci] * in[b][ci][p] over the flat pixels p of a channel plane: a
//                       plain GEMM per image on v_mfma_f32_32x32x2_f32, the weights [Cout][Cin] and the image
//                       [Cin][H W] both as they lie in memory.  Every output is one accumulator's fmaf chain over ci
//                       ascending from +0 (the MFMA is that chain bit for bit: corr_kernel of fmpnp_match.hip with
//                       sparse = weight and dense = in[b]); the zero-padded k tail adds fma(0, 0, acc).  No split-K,
//                       no atomics, so a value does not depend on the tile, the grid or the load width.  Bias, ReLU
//                       and the store are conv3x3_kernel's epilogue (enc::finish).  The image index is part of the
//                       grid: one launch for any B.
//
// The same chain runs on the host in fmpnp_conv1x1_cpu.cpp (the twin).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// A workgroup of 4 waves forms BM output channels x BN flat pixels, each wave 2 x 2 tiles of 32 x 32: 128 x 128
// with the waves 2 x 2, or, for at most 64 output channels, 64 x 256 with the four waves side by side along the
// pixels (conv3x3_kernel's two forms, chosen by the same rule).  k advances BK = 32 input channels at a time.
// Which form runs, and whether the input tile is loaded 16 or 4 bytes at a time, changes no value.
constexpr int BK = 32, C1_NT = 256;
// LDS images, k-major.  Ws[k][m]: the weight tile transposed (a wave's lanes run along k when it is written: the
// odd row stride spreads those writes over the banks).  Xs[k][n]: the input tile as it lies in memory.
template <int MW>  // waves along the output channels: 2 or 1
struct C1Tile {
    static constexpr int BM = 64 * MW, BN = 64 * (4 / MW);
    static constexpr int WS_LD = BM + 1;
    static constexpr int W_PER_T = BM * BK / C1_NT;  // 16 or 8
    static constexpr int X_PER_T = BK * BN / C1_NT;  // 16 or 32
    static_assert(MW == 1 || MW == 2, "four waves: 2 x 2 or 1 x 4");
    static_assert(BM * BK % C1_NT == 0 && BK * BN % (4 * C1_NT) == 0, "both tiles deal out evenly, in float4 too");
};

// VEC: HW % 4 == 0 and `in` is 16-byte aligned, so every channel plane, every pixel tile and every group of four
// pixels of one is; a float4 is then wholly inside the plane or wholly outside.
template <int MW, bool VEC>
__global__ __launch_bounds__(C1_NT) void conv1x1_kernel(const float *__restrict__ in, int Cin, int HW,
                                                        const float *__restrict__ weight,
                                                        const float *__restrict__ bias, int Cout, int flags,
                                                        float *__restrict__ out, int ptiles, int ctiles) {
    using T = C1Tile<MW>;
    constexpr int BM = T::BM, BN = T::BN, WS_LD = T::WS_LD, W_PER_T = T::W_PER_T, X_PER_T = T::X_PER_T;
    __shared__ float Ws[BK * WS_LD];
    __shared__ __attribute__((aligned(16))) float Xs[BK * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block -> (pixel tile, channel tile, image): pixel tiles fastest, so the blocks in flight share one weight tile
    int id = blockIdx.x;
    const int pt = id % ptiles;
    id /= ptiles;
    const int ct = id % ctiles, b = id / ctiles;
    const int p0 = pt * BN, co0 = ct * BM;  // (every tensor is below 2^31 elements: 32-bit offsets within one; a pixel
                                            // index past the plane is formed unsigned)
    const float *img = in + (size_t)b * Cin * HW;

    // global -> register staging.  Weight element e of this thread is (m = e * 8 + tid / 32, k = tid % 32): 32
    // consecutive floats of a weight row per m.  Input element e is flat index e * 256 + tid of the [BK][BN] tile,
    // in floats or, with VEC, in float4 (element e then fills rx[4 e .. 4 e + 3]).  Out-of-range elements are zero.
    const int w_k = tid & 31, w_m = tid >> 5;
    float rw[W_PER_T], rx[X_PER_T];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < W_PER_T; ++e) {
            const int m = co0 + e * 8 + w_m, k = k0 + w_k;
            rw[e] = (m < Cout && k < Cin) ? weight[(size_t)m * Cin + k] : 0.f;
        }
        if constexpr (VEC) {
#pragma unroll
            for (int e = 0; e < X_PER_T / 4; ++e) {
                const int idx = e * C1_NT + tid, k = k0 + idx / (BN / 4);
                const unsigned p = (unsigned)p0 + 4u * (unsigned)(idx % (BN / 4));
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < Cin && p < (unsigned)HW) v = *(const float4 *)(img + (size_t)k * HW + p);
                rx[4 * e] = v.x, rx[4 * e + 1] = v.y, rx[4 * e + 2] = v.z, rx[4 * e + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < X_PER_T; ++e) {
                const int idx = e * C1_NT + tid, k = k0 + idx / BN;
                const unsigned p = (unsigned)p0 + (unsigned)(idx % BN);
                rx[e] = (k < Cin && p < (unsigned)HW) ? img[(size_t)k * HW + p] : 0.f;
            }
        }
    };
    // The MFMA's lanes: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
    const int r = lane & 31, h = lane >> 5;
    const int wm = MW == 2 ? (wave >> 1) * 64 : 0, wn = MW == 2 ? (wave & 1) * 64 : wave * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][bb][g] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < Cin; k0 += BK) {
        __syncthreads();  // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < W_PER_T; ++e) Ws[w_k * WS_LD + e * 8 + w_m] = rw[e];
        if constexpr (VEC) {
#pragma unroll
            for (int e = 0; e < X_PER_T / 4; ++e)  // (flat float4 index idx of [BK][BN / 4] is float 4 idx of [BK][BN])
                *(float4 *)(Xs + 4 * (e * C1_NT + tid)) = make_float4(rx[4 * e], rx[4 * e + 1], rx[4 * e + 2], rx[4 * e + 3]);
        } else {
#pragma unroll
            for (int e = 0; e < X_PER_T; ++e) Xs[e * C1_NT + tid] = rx[e];
        }
        __syncthreads();
        if (k0 + BK < Cin) fetch(k0 + BK);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = Ws[(kk + h) * WS_LD + wm + r], a1 = Ws[(kk + h) * WS_LD + wm + 32 + r];
            const float b0 = Xs[(kk + h) * BN + wn + r], b1 = Xs[(kk + h) * BN + wn + 32 + r];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  The
    // column is the pixel: a wave's lanes store consecutive pixels.
    const bool has_bias = (flags & FMPNP_CONV_BIAS) != 0, do_relu = (flags & FMPNP_CONV_RELU) != 0;
    float *dst = out + (size_t)b * Cout * HW;
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const unsigned p = (unsigned)(p0 + wn + bb * 32 + r);  // (unsigned: HW may be within a tile of 2^31)
        if (p >= (unsigned)HW) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int co = co0 + wm + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
                if (co < Cout)
                    dst[(size_t)co * HW + p] = enc::finish(acc[a][bb][g], has_bias, has_bias ? bias[co] : 0.f, do_relu);
            }
    }
}

}  // namespace

}  // namespace fmpnp

using namespace fmpnp;

namespace {

// validated arguments -> one launch of the <MW> form; 0, FMPNP_ETOOBIG or a hipError_t
template <int MW>
int launch_conv1x1(const float *in, int B, int Cin, int HW, const float *weight, const float *bias, int Cout, int flags,
                   float *out, hipStream_t s) {
    using T = C1Tile<MW>;
    const size_t ptiles = ((size_t)HW + T::BN - 1) / T::BN, ctiles = ((size_t)Cout + T::BM - 1) / T::BM;
    if (ptiles * ctiles > (size_t)INT32_MAX || ptiles * ctiles * (size_t)B > (size_t)INT32_MAX) return FMPNP_ETOOBIG;
    const dim3 grid((unsigned)(ptiles * ctiles * (size_t)B)), block(C1_NT);
    if (HW % 4 == 0 && ((uintptr_t)in & 15) == 0)
        hipLaunchKernelGGL((conv1x1_kernel<MW, true>), grid, block, 0, s, in, Cin, HW, weight, bias, Cout, flags, out,
                           (int)ptiles, (int)ctiles);
    else
        hipLaunchKernelGGL((conv1x1_kernel<MW, false>), grid, block, 0, s, in, Cin, HW, weight, bias, Cout, flags, out,
                           (int)ptiles, (int)ctiles);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int fmpnp_conv1x1_async(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                        int flags, float *out, void *hip_stream) {
    const int rc = enc::conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out, 1);
    if (rc) return rc;
    return Cout <= 64 ? launch_conv1x1<1>(in, B, Cin, H * W, weight, bias, Cout, flags, out, (hipStream_t)hip_stream)
                      : launch_conv1x1<2>(in, B, Cin, H * W, weight, bias, Cout, flags, out, (hipStream_t)hip_stream);
}

int fmpnp_conv1x1(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout, int flags,
                  float *out, void *hip_stream) {
    const int rc = fmpnp_conv1x1_async(in, B, Cin, H, W, weight, bias, Cout, flags, out, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

}  // extern "C"
