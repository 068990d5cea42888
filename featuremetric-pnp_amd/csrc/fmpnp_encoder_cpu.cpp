// fmpnp_encoder_cpu.cpp -- the CPU twins of the encoder's operators (fmpnp_encoder.hip): fmpnp_conv3x3_cpu,
// fmpnp_relu_cpu, fmpnp_maxpool2x2_cpu, with HOST pointers.
//
// The convolution's contract restated for a CPU core: every output is one fp32 fmaf chain over
// k = ci * 9 + ky * 3 + kx ascending from +0 (what v_mfma_f32_32x32x2_f32 computes), a tap outside the image
// being the operand 0, then one fp32 add of the bias and the ReLU.  The chains are fmaf_chains of fmpnp_host.h:
// a block of one output row's pixels is vectorised along x, each pixel its own chain.  fmaf_chains walks a matrix
// with one row per k, so a worker lays the block's taps out as [9 * Cin][XB] once (the shifted, zero-padded input
// rows; only elements inside the image are read) and every output channel runs its chain over it.  The unit is
// built without contraction: the bias add is its own rounding.  Explicit CPU entry points -- parity bridges and
// baselines -- never a fallback of the HIP entry points.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_host.h"

namespace {

constexpr int XB = 64;  // pixels of a row per block: the tap matrix of 512 channels stays near 1 MB

using namespace fmpnp;

}  // namespace

extern "C" int fmpnp_conv3x3_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                                 int Cout, int flags, float *out, int n_threads) {
    const int rc = enc::conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
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
                        const int yy = y + ky - 1;
                        if (yy < 0 || yy >= H) {
                            for (int j = 0; j < nj; ++j) row[j] = 0.f;
                            continue;
                        }
                        const float *src = in + ((size_t)b * Cin + ci) * hw + (size_t)yy * W;
                        for (int j = 0; j < nj; ++j) {
                            const int xx = x0 + j + kx - 1;
                            row[j] = (xx >= 0 && xx < W) ? src[xx] : 0.f;
                        }
                    }
            for (int co = 0; co < Cout; ++co) {
                float *dst = out + ((size_t)b * Cout + co) * hw + (size_t)y * W + x0;
                host::fmaf_chains(weight + (size_t)co * K, taps.data(), (size_t)XB, K, nj, dst);
                const float bv = has_bias ? bias[co] : 0.f;
                for (int j = 0; j < nj; ++j) dst[j] = enc::finish(dst[j], has_bias, bv, do_relu);
            }
        };
    });
    return ok ? 0 : FMPNP_ENOMEM;
}

extern "C" int fmpnp_relu_cpu(const float *in, float *out, long long n, int n_threads) {
    const int rc = enc::relu_args(in, out, n);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    constexpr long long CHUNK = 1 << 16;
    const bool ok = host::deal((n + CHUNK - 1) / CHUNK, n_threads, [&]() {
        return [=](long long c) {
            for (long long i = c * CHUNK, end = std::min(n, i + CHUNK); i < end; ++i) out[i] = enc::relu(in[i]);
        };
    });
    return ok ? 0 : FMPNP_ENOMEM;
}

extern "C" int fmpnp_maxpool2x2_cpu(const float *in, int B, int C, int H, int W, float *out, int n_threads) {
    const int rc = enc::pool_args(in, B, C, H, W, out);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    const int OH = H / 2, OW = W / 2;
    // an item: one output row of one plane
    const bool ok = host::deal((long long)B * C * OH, n_threads, [&]() {
        return [=](long long item) {
            const long long plane = item / OH;
            const int oy = (int)(item % OH);
            const float *r0 = in + (size_t)plane * H * W + (size_t)(2 * oy) * W, *r1 = r0 + W;
            float *dst = out + (size_t)item * OW;
            for (int ox = 0; ox < OW; ++ox) dst[ox] = enc::pool4(r0[2 * ox], r0[2 * ox + 1], r1[2 * ox], r1[2 * ox + 1]);
        };
    }, 16);
    return ok ? 0 : FMPNP_ENOMEM;
}
