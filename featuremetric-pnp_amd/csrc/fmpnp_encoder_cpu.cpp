// fmpnp_encoder_cpu.cpp -- the CPU twins of the encoder's operators (fmpnp_encoder.hip): fmpnp_conv3x3_cpu,
// fmpnp_relu_cpu, fmpnp_maxpool2x2_cpu, with HOST pointers.
//
// The convolution's chain is conv3x3_chains of fmpnp_conv3x3_host.h (shared with the dilated form's twin in
// fmpnp_dense_cpu.cpp), here at dilation 1: every output one fp32 fmaf chain over k = ci * 9 + ky * 3 + kx ascending
// from +0, a tap outside the image being the operand 0, then one fp32 add of the bias and the ReLU.  The unit is
// built without contraction: the bias add is its own rounding.  Explicit CPU entry points -- parity bridges and
// baselines -- never a fallback of the HIP entry points.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_conv3x3_host.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_host.h"

namespace {

constexpr int XB = fmpnp::enc::CONV_XB;  // pixels of a row per block

using namespace fmpnp;

}  // namespace

extern "C" int fmpnp_conv3x3_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                                 int Cout, int flags, float *out, int n_threads) {
    const int rc = enc::conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    return enc::conv3x3_chains(in, B, Cin, H, W, weight, bias, Cout, flags, out, 1, n_threads);
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

// ---- the fp16 precision (include/fmpnp.h, "the encoder's fp16 precision") ----------------------------------
extern "C" size_t fmpnp_conv3x3_f16_weights_size(int Cin, int Cout) { return enc::f16_weight_elems(Cin, Cout) * 2; }

// The GPU pack's image bit for bit: it only converts (host::float_to_half_bits is v_cvt_f16_f32's rounding) and moves.
extern "C" int fmpnp_conv3x3_pack_weights_f16_cpu(const float *weight, int Cin, int Cout, void *packed) {
    const int rc = enc::pack_f16_args(weight, Cin, Cout, packed);
    if (rc) return rc;
    const int CB = enc::f16_cb(Cin), rows = enc::f16_rows(Cout);
    uint16_t *dst = (uint16_t *)packed;
    for (int co = 0; co < rows; ++co)
        for (int cb = 0; cb < CB; ++cb)
            for (int t = 0; t < 9; ++t)
                for (int c = 0; c < 16; ++c) {
                    const int ci = 16 * cb + c;
                    *dst++ = (co < Cout && ci < Cin) ? host::float_to_half_bits(weight[((size_t)co * Cin + ci) * 9 + t])
                                                     : (uint16_t)0;
                }
    return 0;
}

// The REFERENCE of the fp16 convolution (not a twin): fl16 operands, the products accumulated in fp64 in the
// contract's order -- cb ascending, the tap within it, the channel within the step -- one rounding to fp32, then
// the fp32 bias add and the ReLU.  Channels >= Cin and taps outside the image are the operand 0: they are left
// out or add an exact zero.  As in the twin a block of one output row's pixels is vectorised along x: a worker lays
// the block's rounded taps out as [9 Cin][XB] in that order once and every output channel runs over it; the
// weights are rounded once, into the same order.
extern "C" int fmpnp_conv3x3_f16_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                                     int Cout, int flags, float *out, int n_threads) {
    const int rc = enc::conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out);
    if (rc) return rc;
    if (enc::f16_weight_elems(Cin, Cout) == 0) return FMPNP_ETOOBIG;
    if (n_threads < 0) return FMPNP_EINVAL;
    const bool has_bias = (flags & FMPNP_CONV_BIAS) != 0, do_relu = (flags & FMPNP_CONV_RELU) != 0;
    const int K = 9 * Cin, CB = enc::f16_cb(Cin), xblocks = (W + XB - 1) / XB;
    const size_t hw = (size_t)H * W;
    // row `o` of the order is (ci, t): o runs over cb, then t, then the channels of cb below Cin
    std::vector<int> order_ci, order_t;
    std::vector<float> w16;
    try {
        order_ci.reserve(K), order_t.reserve(K);
        for (int cb = 0; cb < CB; ++cb)
            for (int t = 0; t < 9; ++t)
                for (int ci = 16 * cb; ci < std::min(Cin, 16 * cb + 16); ++ci) order_ci.push_back(ci), order_t.push_back(t);
        w16.resize((size_t)Cout * K);
    } catch (...) {
        return FMPNP_ENOMEM;
    }
    for (int co = 0; co < Cout; ++co)
        for (int o = 0; o < K; ++o)
            w16[(size_t)co * K + o] = host::fl16(weight[((size_t)co * Cin + order_ci[o]) * 9 + order_t[o]]);
    const int *oci = order_ci.data(), *ot = order_t.data();
    const float *wr = w16.data();
    // an item: (image b, row y, block of XB pixels)
    const bool ok = host::deal((long long)B * H * xblocks, n_threads, [&]() {
        return [=, taps = std::vector<float>((size_t)K * XB)](long long item) mutable {
            const int xb = (int)(item % xblocks), y = (int)(item / xblocks % H), b = (int)(item / xblocks / H);
            const int x0 = xb * XB, nj = std::min(XB, W - x0);
            for (int o = 0; o < K; ++o) {
                float *row = taps.data() + (size_t)o * XB;
                const int ky = ot[o] / 3, kx = ot[o] % 3, yy = y + ky - 1;
                if (yy < 0 || yy >= H) {
                    for (int j = 0; j < nj; ++j) row[j] = 0.f;
                    continue;
                }
                const float *src = in + ((size_t)b * Cin + oci[o]) * hw + (size_t)yy * W;
                for (int j = 0; j < nj; ++j) {
                    const int xx = x0 + j + kx - 1;
                    row[j] = (xx >= 0 && xx < W) ? host::fl16(src[xx]) : 0.f;
                }
            }
            double acc[XB];
            for (int co = 0; co < Cout; ++co) {
                const float *wk = wr + (size_t)co * K;
                for (int j = 0; j < nj; ++j) acc[j] = 0.0;
                for (int o = 0; o < K; ++o) {
                    const double w = (double)wk[o];
                    const float *row = taps.data() + (size_t)o * XB;
                    for (int j = 0; j < nj; ++j) acc[j] += w * (double)row[j];  // (the product is exact in fp64)
                }
                float *dst = out + ((size_t)b * Cout + co) * hw + (size_t)y * W + x0;
                const float bv = has_bias ? bias[co] : 0.f;
                for (int j = 0; j < nj; ++j) dst[j] = enc::finish((float)acc[j], has_bias, bv, do_relu);
            }
        };
    });
    return ok ? 0 : FMPNP_ENOMEM;
}
