// fmpnp_dense_cpu.cpp -- the CPU twins of the dense-feature operators (include/fmpnp.h, "dense features"), with HOST
// pointers: fmpnp_conv3x3_dilated_cpu (conv3x3_kernel<MW, D> of fmpnp_encoder.hip), fmpnp_avgpool2x2s1_cpu and
// fmpnp_dense_pyramid_step_cpu (fmpnp_dense.hip).
//
// The convolution's chain is conv3x3_chains of fmpnp_conv3x3_host.h, which fmpnp_conv3x3_cpu runs at dilation 1.  The
// pool and the pyramid step form every value with the functions of the *_impl.h headers the kernels are built from,
// and this unit is compiled without contraction and without -mfma (fma() is libm's, correctly rounded): each
// * + / sqrt rounds as the GPU's does and the squares are summed in the contract's order, so every output element is
// the GPU's bit for bit.  Explicit CPU entry points -- parity bridges and baselines -- never a fallback of the HIP
// entry points.
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_conv3x3_host.h"
#include "fmpnp_dense_impl.h"
#include "fmpnp_host.h"

using namespace fmpnp;

extern "C" int fmpnp_conv3x3_dilated_cpu(const float *in, int B, int Cin, int H, int W, const float *weight,
                                         const float *bias, int Cout, int flags, float *out, int dilation, int n_threads) {
    const int rc = enc::conv_dilated_args(in, B, Cin, H, W, weight, bias, Cout, flags, out, dilation);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    return enc::conv3x3_chains(in, B, Cin, H, W, weight, bias, Cout, flags, out, dilation, n_threads);
}

extern "C" int fmpnp_avgpool2x2s1_cpu(const float *in, int B, int C, int H, int W, float *out, int n_threads) {
    const int rc = enc::pool_args(in, B, C, H, W, out);
    if (rc) return rc;
    if (n_threads < 0) return FMPNP_EINVAL;
    const int OH = H - 1, OW = W - 1;
    // an item: one output row of one plane
    const bool ok = host::deal((long long)B * C * OH, n_threads, [&]() {
        return [=](long long item) {
            const long long plane = item / OH;
            const int oy = (int)(item % OH);
            const float *r0 = in + (size_t)plane * H * W + (size_t)oy * W, *r1 = r0 + W;
            float *dst = out + (size_t)item * OW;
            for (int ox = 0; ox < OW; ++ox) dst[ox] = enc::avg4(r0[ox], r0[ox + 1], r1[ox], r1[ox + 1]);
        };
    }, 16);
    return ok ? 0 : FMPNP_ENOMEM;
}

namespace {

using namespace fmpnp::hc;

struct Step {
    const float *cur, *prev;
    float *out;
    int C, h, w, hp, wp;
    bool norm;
};

// v[x], x in [0, w): the step's values of channel c of row (b, y) before the division
void value_row(const Step &k, const Tap *tx, int b, int y, int c, float *v) {
    const size_t plane = (size_t)b * (size_t)k.C + (size_t)c;
    const float *cr = k.cur + (plane * (size_t)k.h + (size_t)y) * (size_t)k.w;
    if (!k.prev) {
        for (int x = 0; x < k.w; ++x) v[x] = cr[x];
        return;
    }
    const Tap ty = axis_tap(axis_scale(k.hp, k.h), k.hp, y);
    const float *pp = k.prev + plane * (size_t)k.hp * (size_t)k.wp;
    const float *p0 = pp + (size_t)ty.i0 * (size_t)k.wp, *p1 = pp + (size_t)ty.i1 * (size_t)k.wp;
    for (int x = 0; x < k.w; ++x) {
        const Tap &t = tx[x];
        v[x] = dense::summed(cr[x], bilerp(p0[t.i0], p0[t.i1], p1[t.i0], p1[t.i1], t.w0, t.w1, ty.w0, ty.w1));
    }
}

// (out may be cur: the row's pass 1 is over before its first store, and pass 2 reads a channel's row before it
// writes it)
void do_row(const Step &k, const Tap *tx, int b, int y, float *v, double *acc, double *sum, float *dv) {
    const int w = k.w;
    if (k.norm) {
        std::fill(sum, sum + w, 0.0);
        for (int c0 = 0; c0 < k.C; c0 += BLOCK) {
            std::fill(acc, acc + w, 0.0);
            for (int c = c0; c < std::min(k.C, c0 + BLOCK); ++c) {
                value_row(k, tx, b, y, c, v);
                for (int x = 0; x < w; ++x) acc[x] = square_acc(v[x], acc[x]);
            }
            for (int x = 0; x < w; ++x) sum[x] = sum[x] + acc[x];
        }
        for (int x = 0; x < w; ++x) dv[x] = dense::divisor(norm_of(sum[x]));
    }
    for (int c = 0; c < k.C; ++c) {
        value_row(k, tx, b, y, c, v);
        float *o = k.out + (((size_t)b * (size_t)k.C + (size_t)c) * (size_t)k.h + (size_t)y) * (size_t)w;
        if (k.norm)
            for (int x = 0; x < w; ++x) o[x] = normalised(v[x], dv[x]);
        else
            for (int x = 0; x < w; ++x) o[x] = v[x];
    }
}

}  // namespace

extern "C" int fmpnp_dense_pyramid_step_cpu(const float *cur, const float *prev, int B, int C, int h, int w, int hp,
                                            int wp, float *out, int flags, int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    const int rc = dense::step_args(cur, prev, B, C, h, w, hp, wp, out, flags);
    if (rc) return rc;
    const Step k{cur, prev, out, C, h, w, prev ? hp : 1, prev ? wp : 1, (flags & FMPNP_PYR_NORMALIZE) != 0};
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        std::vector<Tap> tx((size_t)w);
        const float sx = axis_scale(k.wp, w);
        for (int x = 0; x < w; ++x) tx[(size_t)x] = axis_tap(sx, k.wp, x);
        const Tap *txp = tx.data();
        const bool ok = host::deal((long long)B * h, n_threads, [&]() {
            return [&k, txp, h, v = std::vector<float>((size_t)w), dv = std::vector<float>((size_t)w),
                    acc = std::vector<double>((size_t)w), sum = std::vector<double>((size_t)w)](long long r) mutable {
                do_row(k, txp, (int)(r / h), (int)(r % h), v.data(), acc.data(), sum.data(), dv.data());
            };
        });
        if (!ok) return FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
    return 0;
}
