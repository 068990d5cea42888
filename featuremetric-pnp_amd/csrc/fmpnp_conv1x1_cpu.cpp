// fmpnp_conv1x1_cpu.cpp -- the CPU twin of the 1x1 convolution (fmpnp_conv1x1.hip): fmpnp_conv1x1_cpu, with HOST
// pointers.
//
// The contract restated for a CPU core: every output is one fp32 fmaf chain over ci ascending from +0 (what
// v_mfma_f32_32x32x2_f32 computes), then one fp32 add of the bias and the ReLU (enc::finish).  The chains are
// fmaf_chains of fmpnp_host.h: a block of PB flat pixels is vectorised along the pixels, each pixel its own chain.
// fmaf_chains walks a matrix with one row per k, and the image [Cin][H W] is that matrix as it lies in memory, so
// nothing is laid out.  The unit is built without contraction: the bias add is its own rounding.  An explicit CPU
// entry point -- a parity bridge and a baseline -- never a fallback of the HIP entry point.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_host.h"

namespace {

constexpr int PB = 256;  // pixels per block: its accumulators and one row of the image stay in L1

using namespace fmpnp;

}  // namespace

extern "C" int fmpnp_conv1x1_cpu(const float *in, int B, int Cin, int H, int W, const float *weight, const float *bias,
                                 int Cout, int flags, float *out, int n_threads) {
    const int rc = enc::conv_args(in, B, Cin, H, W, weight, bias, Cout, flags, out, 1);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    const bool has_bias = (flags & FMPNP_CONV_BIAS) != 0, do_relu = (flags & FMPNP_CONV_RELU) != 0;
    const size_t hw = (size_t)H * W;
    const long long pblocks = (long long)((hw + PB - 1) / PB);
    // an item: (image b, block of PB pixels)
    const bool ok = host::deal((long long)B * pblocks, n_threads, [&]() {
        return [=](long long item) {
            const int b = (int)(item / pblocks);
            const size_t p0 = (size_t)(item % pblocks) * PB;
            const int nj = (int)std::min<size_t>(PB, hw - p0);
            const float *src = in + (size_t)b * Cin * hw + p0;
            for (int co = 0; co < Cout; ++co) {
                float *dst = out + ((size_t)b * Cout + co) * hw + p0;
                host::fmaf_chains(weight + (size_t)co * Cin, src, hw, Cin, nj, dst);
                const float bv = has_bias ? bias[co] : 0.f;
                for (int j = 0; j < nj; ++j) dst[j] = enc::finish(dst[j], has_bias, bv, do_relu);
            }
        };
    });
    return ok ? 0 : FMPNP_ENOMEM;
}
