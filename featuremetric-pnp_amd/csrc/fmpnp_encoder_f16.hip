// fmpnp_encoder_f16.hip -- the opt-in fp16 precision of the encoder's 3x3 convolution on gfx950 (include/fmpnp.h,
// "the encoder's fp16 precision").  The exact-fp32 kernels of fmpnp_encoder.hip are not touched.
//
//   pack_weights_kernel  fp32 weights [Cout][Cin][3][3] -> the fp16 image [Cout_p][CB][9][16] (CB = ceil(Cin / 16),
//                        Cout_p = Cout up to a multiple of 32, zero tails): one thread per 16-byte unit of 8
//                        channels, rounded with v_cvt_f16_f32 (nearest-even).  Once per weight, not per launch.
//   conv3x3_f16_kernel   out[co][pixel] = sum over steps st = cb * 9 + tap ascending of the 16 products of the
//                        channels 16 cb .. 16 cb + 15 at that tap: an implicit GEMM on v_mfma_f32_32x32x16_f16, one
//                        fp32 accumulator per output from +0, no split-K, no atomics, so a value does not depend on
//                        the tile or the grid.  A k tile is one cb: 16 whole channels, 9 MFMA steps.  The weight
//                        tile comes from the packed image in 16-byte units (a lane's A fragment is one unit); the
//                        tap operand is never formed: the block stages the fp32 input halo of its pixel tile,
//                        rounds it to fp16 on the way (v_cvt_f16_f32) and writes 8 channels of one halo position as
//                        one 16-byte unit, so a lane's B fragment is one ds_read_b128 at tap shift + pixel.  Bias,
//                        ReLU and the stores along the pixel are the exact kernel's epilogue (enc::finish).
//
// The CPU reference (not a twin: the order inside one MFMA is undocumented) and the bit-identical CPU weight pack
// are in fmpnp_encoder_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // a 16-byte unit: 8 fp16 values

constexpr int PACK_NT = 256;

// unit u of the image: (co, cb, t, h) = the channels 16 cb + 8 h .. + 7 of tap t of output channel co
__global__ __launch_bounds__(PACK_NT) void pack_weights_kernel(const float *__restrict__ weight, int Cin, int Cout, int CB,
                                                               u32x4 *__restrict__ packed, long long units) {
    const long long u = (long long)blockIdx.x * PACK_NT + threadIdx.x;
    if (u >= units) return;
    const int h = (int)(u & 1);
    long long q = u >> 1;
    const int t = (int)(q % 9);
    q /= 9;
    const int cb = (int)(q % CB), co = (int)(q / CB);
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = 16 * cb + 8 * h + j;
        v[j] = (_Float16)((co < Cout && ci < Cin) ? weight[((size_t)co * Cin + ci) * 9 + t] : 0.f);
    }
    packed[u] = __builtin_bit_cast(u32x4, v);
}

// ---- convolution --------------------------------------------------------------------------------
// The exact kernel's decompositions: a workgroup of 4 waves forms BM output channels x BN pixels, each wave 2 x 2
// tiles of 32 x 32: 128 x 128 with the waves 2 x 2, or, for layers of at most 64 output channels, 64 x 256 with the
// four waves side by side along the pixels.  Which form runs changes no value.  The pixel tile is TR rows x TW
// columns of the image, TW = 1 << lw in 4 .. BN and TR = BN / TW; pixel n of the tile is (n >> lw, n & (TW - 1)).
// k advances one cb (16 input channels, 9 MFMA steps of 16) at a time.
constexpr int CONV_NT = 256, A_UNITS_ROW = 18;  // the 16-byte units of one output channel's k tile: [tap][h]
// LDS images in 16-byte units.  As[q = 2 tap + h][m], row stride BM + 1: the 16 lanes of a write group run along q
// of one weight row (its 288 bytes are contiguous in the image) and fall on 16 different 16-byte bank slots; a read
// group is 32 consecutive units.  Hs[h][hy][hx]: the halo, (TR + 2) x (TW + 2) positions per 8 channels, at most
// 3 x (BN + 2); written and read along x.
template <int MW>  // waves along the output channels: 2 or 1
struct ConvTileH {
    static constexpr int BM = 64 * MW, BN = 64 * (4 / MW);
    static constexpr int LW_MAX = BN == 128 ? 7 : 8;
    static constexpr int AS_LD = BM + 1;
    static constexpr int HALO_MAX = 3 * (BN + 2);                                   // (TR + 2)(TW + 2): largest at TW = BN
    static constexpr int A_PER_T = (BM * A_UNITS_ROW + CONV_NT - 1) / CONV_NT;      // 9 or 5 (the last half used)
    static constexpr int H_PER_T = (2 * HALO_MAX + CONV_NT - 1) / CONV_NT;          // 4 or 7
    static_assert(MW == 1 || MW == 2, "four waves: 2 x 2 or 1 x 4");
};

template <int MW>
__global__ __launch_bounds__(CONV_NT) void conv3x3_f16_kernel(const float *__restrict__ in, int Cin, int H, int W,
                                                              const u32x4 *__restrict__ packed, int rows_p,
                                                              const float *__restrict__ bias, int Cout, int flags,
                                                              float *__restrict__ out, int lw, int tiles_x, int ptiles,
                                                              int ctiles) {
    using T = ConvTileH<MW>;
    constexpr int BM = T::BM, BN = T::BN, AS_LD = T::AS_LD, HALO_MAX = T::HALO_MAX, A_PER_T = T::A_PER_T,
                  H_PER_T = T::H_PER_T;
    __shared__ u32x4 As[A_UNITS_ROW * AS_LD];
    __shared__ u32x4 Hs[2 * HALO_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block -> (pixel tile, channel tile, image): pixel tiles fastest, so the blocks in flight share one weight tile
    int id = blockIdx.x;
    const int pt = id % ptiles;
    id /= ptiles;
    const int ct = id % ctiles, b = id / ctiles;
    const int TW = 1 << lw, TR = BN >> lw, RS = TW + 2, CS = (TR + 2) * RS;  // halo row stride, positions per 8 channels
    const int y0 = (pt / tiles_x) * TR, x0 = (pt % tiles_x) * TW, co0 = ct * BM;
    const int HW = H * W, CB = (Cin + 15) >> 4;  // (every tensor is below 2^31 elements: 32-bit offsets within one)
    const float *img = in + (size_t)b * Cin * HW;

    // global -> register staging.  Weight unit e of this thread is flat index e * 256 + tid of the [BM][18] tile:
    // (m, q) = (idx / 18, idx % 18), the 18 consecutive units of row co0 + m of the image at this cb; rows the image
    // does not have (>= rows_p) are zero.  Halo unit e is flat index e * 256 + tid of [2][TR + 2][TW + 2]: the
    // channels 8 h .. 8 h + 7 of the k tile at one halo position.  The position's place in the image does not change
    // from k tile to k tile, so the offset is formed once: hoff = y * W + x, or -1 outside the image (or past the
    // halo).  The 8 channels are 8 dword loads HW apart; a wave's lanes run along x.
    int hoff[H_PER_T], hh[H_PER_T];
#pragma unroll
    for (int e = 0; e < H_PER_T; ++e) {
        const int idx = e * CONV_NT + tid;
        const int h8 = idx / CS, rem = idx - h8 * CS, hy = rem / RS, hx = rem - hy * RS;
        const int y = y0 + hy - 1, x = x0 + hx - 1;
        const bool inside = h8 < 2 && y >= 0 && y < H && x >= 0 && x < W;
        hh[e] = h8;
        hoff[e] = inside ? y * W + x : -1;
    }
    int aoff[A_PER_T];  // the unit's place in the image less the cb term, or -1
#pragma unroll
    for (int e = 0; e < A_PER_T; ++e) {
        const int idx = e * CONV_NT + tid, m = idx / A_UNITS_ROW, q = idx - m * A_UNITS_ROW;
        aoff[e] = (m < BM && co0 + m < rows_p) ? q : -1;
    }
    u32x4 ra[A_PER_T];
    float rh[H_PER_T][8];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    auto fetch = [&](int cb) {  // the k tile of input channels 16 cb .. 16 cb + 15
#pragma unroll
        for (int e = 0; e < A_PER_T; ++e) {
            const int idx = e * CONV_NT + tid, m = idx / A_UNITS_ROW;
            ra[e] = aoff[e] >= 0 ? packed[((size_t)(co0 + m) * CB + cb) * A_UNITS_ROW + aoff[e]] : zero;
        }
#pragma unroll
        for (int e = 0; e < H_PER_T; ++e) {
            const int c0 = 16 * cb + 8 * hh[e];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                rh[e][j] = (hoff[e] >= 0 && c0 + j < Cin) ? img[(size_t)(c0 + j) * HW + hoff[e]] : 0.f;
        }
    };
    // The MFMA's lanes: A[i = lane & 31][k = 8 (lane >> 5) + j], B[k = 8 (lane >> 5) + j][col = lane & 31], j = 0 .. 7:
    // k is the channel within the cb, so a lane's fragment is the unit h = lane >> 5.  The halo offset of a tap is
    // (ky, kx) in the halo's strides, the same for every k tile, plus the lane's pixel.
    const int r = lane & 31, h = lane >> 5;
    const int wm = MW == 2 ? (wave >> 1) * 64 : 0, wn = MW == 2 ? (wave & 1) * 64 : wave * 64;
    int pix[2];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int n = wn + bb * 32 + r;
        pix[bb] = h * CS + (n >> lw) * RS + (n & (TW - 1));  // halo (ty + ky, tx + kx) is the tap (ky - 1, kx - 1) of the pixel
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][bb][g] = 0.f;
    fetch(0);
    for (int cb = 0; cb < CB; ++cb) {
        __syncthreads();  // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < A_PER_T; ++e) {
            const int idx = e * CONV_NT + tid, m = idx / A_UNITS_ROW, q = idx - m * A_UNITS_ROW;
            if (m < BM) As[q * AS_LD + m] = ra[e];
        }
#pragma unroll
        for (int e = 0; e < H_PER_T; ++e) {
            const int idx = e * CONV_NT + tid;
            f16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (_Float16)rh[e][j];  // v_cvt_f16_f32: round-to-nearest-even
            if (idx < 2 * CS) Hs[idx] = __builtin_bit_cast(u32x4, v);
        }
        __syncthreads();
        if (cb + 1 < CB) fetch(cb + 1);  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int q = 2 * t + h, tap = (t / 3) * RS + (t % 3);
            const f16x8 a0 = __builtin_bit_cast(f16x8, As[q * AS_LD + wm + r]);
            const f16x8 a1 = __builtin_bit_cast(f16x8, As[q * AS_LD + wm + 32 + r]);
            const f16x8 b0 = __builtin_bit_cast(f16x8, Hs[tap + pix[0]]);
            const f16x8 b1 = __builtin_bit_cast(f16x8, Hs[tap + pix[1]]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
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

}  // namespace

}  // namespace fmpnp

using namespace fmpnp;

namespace {

// validated arguments -> one launch of the <MW> form; 0, FMPNP_ETOOBIG or a hipError_t
template <int MW>
int launch_conv_f16(const float *in, int B, int Cin, int H, int W, const void *packed, const float *bias, int Cout,
                    int flags, float *out, hipStream_t s) {
    using T = ConvTileH<MW>;
    int lw = 2;  // TW = 4 at least; the smallest power of two that holds a row, BN at most
    while (lw < T::LW_MAX && (1 << lw) < W) ++lw;
    const int TW = 1 << lw, TR = T::BN >> lw;
    const size_t tiles_x = ((size_t)W + TW - 1) / TW, tiles_y = ((size_t)H + TR - 1) / TR;
    const size_t ptiles = tiles_x * tiles_y, ctiles = ((size_t)Cout + T::BM - 1) / T::BM;
    if (ptiles > (size_t)INT32_MAX || ptiles * ctiles > (size_t)INT32_MAX || ptiles * ctiles * (size_t)B > (size_t)INT32_MAX)
        return FMPNP_ETOOBIG;
    hipLaunchKernelGGL(conv3x3_f16_kernel<MW>, dim3((unsigned)(ptiles * ctiles * (size_t)B)), dim3(CONV_NT), 0, s, in, Cin,
                       H, W, (const u32x4 *)packed, enc::f16_rows(Cout), bias, Cout, flags, out, lw, (int)tiles_x,
                       (int)ptiles, (int)ctiles);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int fmpnp_conv3x3_pack_weights_f16_async(const float *weight, int Cin, int Cout, void *packed, void *hip_stream) {
    const int rc = enc::pack_f16_args(weight, Cin, Cout, packed);
    if (rc) return rc;
    const int CB = enc::f16_cb(Cin);
    const long long units = (long long)enc::f16_rows(Cout) * CB * 9 * 2;  // (< 2^28: the image is below 2^31 elements)
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((units + PACK_NT - 1) / PACK_NT)), dim3(PACK_NT), 0,
                       (hipStream_t)hip_stream, weight, Cin, Cout, CB, (u32x4 *)packed, units);
    return (int)hipGetLastError();
}

int fmpnp_conv3x3_f16_async(const float *in, int B, int Cin, int H, int W, const void *packed, const float *bias, int Cout,
                            int flags, float *out, void *hip_stream) {
    const int rc = enc::conv_f16_args(in, B, Cin, H, W, packed, bias, Cout, flags, out);
    if (rc) return rc;
    return Cout <= 64 ? launch_conv_f16<1>(in, B, Cin, H, W, packed, bias, Cout, flags, out, (hipStream_t)hip_stream)
                      : launch_conv_f16<2>(in, B, Cin, H, W, packed, bias, Cout, flags, out, (hipStream_t)hip_stream);
}

int fmpnp_conv3x3_f16(const float *in, int B, int Cin, int H, int W, const void *packed, const float *bias, int Cout,
                      int flags, float *out, void *hip_stream) {
    const int rc = fmpnp_conv3x3_f16_async(in, B, Cin, H, W, packed, bias, Cout, flags, out, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

}  // extern "C"
