// fmpnp_conv3x3_host.h -- the 3x3 convolution's chain on a CPU core, shared by its twins: fmpnp_conv3x3_cpu
// (fmpnp_encoder_cpu.cpp, dilation 1) and fmpnp_conv3x3_dilated_cpu (fmpnp_dense_cpu.cpp).
//
// The contract restated: every output is one fp32 fmaf chain over k = ci * 9 + ky * 3 + kx ascending from +0 (what
// v_mfma_f32_32x32x2_f32 computes), tap (ky, kx) of pixel (y, x) being the input at (y + (ky - 1) d, x + (kx - 1) d)
// or, outside the image, the operand 0; then one fp32 add of the bias and the ReLU (enc::finish).  The chains are
// fmaf_chains of fmpnp_host.h: a block of one output row's pixels is vectorised along x, each pixel its own chain.
// fmaf_chains walks a matrix with one row per k, so a worker lays the block's taps out as [9 * Cin][XB] once (the
// shifted, zero-padded input rows; only elements inside the image are read) and every output channel runs its
// chain over it.  The including unit is built without contraction: the bias add is its own rounding.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_host.h"

namespace fmpnp {
namespace enc {

constexpr int CONV_XB = 64;  // pixels of a row per block: the tap matrix of 512 channels stays near 1 MB

// validated arguments (enc::conv_args; d >= 1) -> 0 or FMPNP_ENOMEM
inline int conv3x3_chains(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias, int Cout,
                          int flags, float *out, int d, int n_threads) {
    constexpr int XB = CONV_XB;
    const bool has_bias = (flags & FMPNP_CONV_BIAS) != 0, do_relu = (flags & FMPNP_CONV_RELU) != 0;
    const int K = 9 * Cin, xblocks = (W + XB - 1) / XB;
    const size_t hw = (size_t)H * W;
    // an item: (image b, row y, block of XB pixels)
    const bool ok = host::deal((long long)B * H * xblocks, n_threads, [&]() {
        return [=, taps = std::vector<float>((size_t)K * XB)](long long item) mutable {
            const int xb = (int)(item % xblocks), y = (int)(item / xblocks % H), b = (int)(item / xblocks / H);
            const int x0 = xb * XB, nj = std::min(XB, W - x0);
            for (int ci = 0; ci < Cin; ++ci)
                for (int ky = 0; ky < 3; ++ky)
                    for (int kx = 0; kx < 3; ++kx) {
                        float *row = taps.data() + (size_t)(ci * 9 + ky * 3 + kx) * XB;
                        const int yy = y + (ky - 1) * d;
                        if (yy < 0 || yy >= H) {
                            for (int j = 0; j < nj; ++j) row[j] = 0.f;
                            continue;
                        }
                        const float *src = in + ((size_t)b * Cin + ci) * hw + (size_t)yy * W;
                        for (int j = 0; j < nj; ++j) {
                            const int xx = x0 + j + (kx - 1) * d;
                            row[j] = (xx >= 0 && xx < W) ? src[xx] : 0.f;
                        }
                    }
            for (int co = 0; co < Cout; ++co) {
                float *dst = out + ((size_t)b * Cout + co) * hw + (size_t)y * W + x0;
                host::fmaf_chains(weight + (size_t)co * K, taps.data(), (size_t)XB, K, nj, dst);
                const float bv = has_bias ? bias[co] : 0.f;
                for (int j = 0; j < nj; ++j) dst[j] = finish(dst[j], has_bias, bv, do_relu);
            }
        };
    });
    return ok ? 0 : FMPNP_ENOMEM;
}

}  // namespace enc
}  // namespace fmpnp
