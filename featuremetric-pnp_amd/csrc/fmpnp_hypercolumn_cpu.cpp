// fmpnp_hypercolumn_cpu.cpp -- fmpnp_hypercolumn_assemble_cpu: the CPU twin of fmpnp_hypercolumn_assemble
// (s2dhm/network/network.py:149-173) with HOST pointers.
//
// Every value comes from fmpnp_hypercolumn_impl.h, the header the kernel of fmpnp_hypercolumn.hip is built
// from, and this unit is compiled without contraction and without -mfma (fma() is libm's, correctly
// rounded): each * + / sqrt rounds as the GPU's does and the squares are summed in the contract's order
// (a chain per 64-channel block, the blocks in ascending order), so every output element is the GPU's bit
// for bit.  The output rows are independent; they are dealt over the host threads.  An explicit CPU entry
// point -- a parity bridge and a baseline -- never a fallback of the HIP entry points.
#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_hypercolumn_impl.h"

namespace {

using namespace fmpnp::hc;

struct Call {
    const fmpnp_hc_layer *layers;
    int L, B, H, W;
    long long C;
    float *out;
    size_t osb, osc, osy;
    bool norm;
};

// every layer's taps along x for every output column
struct RowGeo {
    std::vector<Tap> tx;  // [L][W]
};

// the resized values of row (b, y) of one layer's channel c: v[x] for x in [0, W)
void resize_row(const fmpnp_hc_layer &ly, int b, int c, const Tap &ty, const Tap *tx, int W, float *v) {
    const float *plane = ly.data + (size_t)b * (size_t)ly.stride_b + (size_t)c * (size_t)ly.stride_c;
    const float *p0 = plane + (size_t)ty.i0 * (size_t)ly.stride_y, *p1 = plane + (size_t)ty.i1 * (size_t)ly.stride_y;
    for (int x = 0; x < W; ++x) {
        const Tap &t = tx[x];
        v[x] = bilerp(p0[t.i0], p0[t.i1], p1[t.i0], p1[t.i1], t.w0, t.w1, ty.w0, ty.w1);
    }
}

// body(c, v): the values v[W] of concatenated channel c of row (b, y), for c in [c_begin, c_end) ascending
template <class F>
void walk(const Call &k, const RowGeo &g, int b, int y, long long c_begin, long long c_end, float *v, F &&body) {
    long long first = 0;
    for (int l = 0; l < k.L && first < c_end; ++l) {
        const fmpnp_hc_layer &ly = k.layers[l];
        const long long lo = std::max(c_begin, first), hi = std::min(c_end, first + ly.C);
        if (lo < hi) {
            const Tap ty = axis_tap(axis_scale(ly.H, k.H), ly.H, y);
            for (long long c = lo; c < hi; ++c) {
                resize_row(ly, b, (int)(c - first), ty, &g.tx[(size_t)l * (size_t)k.W], k.W, v);
                body(c, v);
            }
        }
        first += ly.C;
    }
}

void do_row(const Call &k, const RowGeo &g, int b, int y, float *v, double *acc, double *sum, float *n) {
    const int W = k.W;
    if (k.norm) {
        std::fill(sum, sum + W, 0.0);
        for (long long c0 = 0; c0 < k.C; c0 += BLOCK) {
            std::fill(acc, acc + W, 0.0);
            walk(k, g, b, y, c0, std::min(k.C, c0 + BLOCK), v, [&](long long, const float *vv) {
                for (int x = 0; x < W; ++x) acc[x] = square_acc(vv[x], acc[x]);
            });
            for (int x = 0; x < W; ++x) sum[x] = sum[x] + acc[x];
        }
        for (int x = 0; x < W; ++x) n[x] = norm_of(sum[x]);
    }
    float *orow = k.out + (size_t)b * k.osb + (size_t)y * k.osy;
    walk(k, g, b, y, 0, k.C, v, [&](long long c, const float *vv) {
        float *o = orow + (size_t)c * k.osc;
        if (k.norm)
            for (int x = 0; x < W; ++x) o[x] = normalised(vv[x], n[x]);
        else
            for (int x = 0; x < W; ++x) o[x] = vv[x];
    });
}

}  // namespace

extern "C" int fmpnp_hypercolumn_assemble_cpu(const fmpnp_hc_layer *layers, int L, int B, float *out, int H, int W,
                                              long long out_stride_b, long long out_stride_c, long long out_stride_y,
                                              int flags, int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    long long C = 0;
    const int rc = check_args(layers, L, B, out, H, W, out_stride_b, out_stride_c, out_stride_y, flags, &C);
    if (rc) return rc;
    const Call k{layers, L, B, H, W, C, out, (size_t)out_stride_b, (size_t)out_stride_c, (size_t)out_stride_y,
                 (flags & FMPNP_HC_NORMALIZE) != 0};
    const long long rows = (long long)B * H;
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        RowGeo g;
        g.tx.resize((size_t)L * (size_t)W);
        for (int l = 0; l < L; ++l) {
            const float sx = axis_scale(layers[l].W, W);
            for (int x = 0; x < W; ++x) g.tx[(size_t)l * (size_t)W + (size_t)x] = axis_tap(sx, layers[l].W, x);
        }
        const bool ok = fmpnp::host::deal(rows, n_threads, [&]() {
            return [&k, &g, H, v = std::vector<float>((size_t)W), n = std::vector<float>((size_t)W),
                    acc = std::vector<double>((size_t)W), sum = std::vector<double>((size_t)W)](long long r) mutable {
                do_row(k, g, (int)(r / H), (int)(r % H), v.data(), acc.data(), sum.data(), n.data());
            };
        });
        if (!ok) return FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
    return 0;
}
