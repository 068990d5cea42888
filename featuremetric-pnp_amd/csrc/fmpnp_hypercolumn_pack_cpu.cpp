// fmpnp_hypercolumn_pack_cpu.cpp -- fmpnp_hypercolumn_pack_cpu: the CPU twin of fmpnp_hypercolumn_pack with HOST
// pointers.
//
// Every value comes from fmpnp_hypercolumn_impl.h and fmpnp_hypercolumn_pack_impl.h, the headers the kernels of
// fmpnp_hypercolumn_pack.hip are built from, and this unit is compiled without contraction and without -mfma, so
// every element written is the GPU's bit for bit.  First the norm of every texel (over all channels, the
// assembly's block order), then the output rows, both dealt over the host threads: a row forms the (padded)
// rows y - 1, y, y + 1 of each channel of the range and slides the Sobel's window along them.  An explicit CPU
// entry point -- a parity bridge and a yardstick -- never a fallback of the HIP entry points.
#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_hypercolumn_pack_impl.h"

namespace {

using namespace fmpnp::hc;
using namespace fmpnp::hcp;

struct Call {
    const fmpnp_hc_layer *layers;
    int L, item, H, W;
    long long C;
    int c_begin, c_end, cs;
    bool norm, grad, f64, sn, replicate;
    const unsigned char *marks;
    void *out;
    std::vector<Tap> tx;   // [L][W]
    std::vector<float> n;  // [H][W] (norm)
};

// the resized values of row y of layer l's channel c: v[x] for x in [0, W)
void resize_row(const Call &k, int l, int c, int y, float *v) {
    const fmpnp_hc_layer &ly = k.layers[l];
    const Tap ty = axis_tap(axis_scale(ly.H, k.H), ly.H, y);
    const float *plane = ly.data + (size_t)k.item * (size_t)ly.stride_b + (size_t)c * (size_t)ly.stride_c;
    const float *p0 = plane + (size_t)ty.i0 * (size_t)ly.stride_y, *p1 = plane + (size_t)ty.i1 * (size_t)ly.stride_y;
    const Tap *tx = &k.tx[(size_t)l * (size_t)k.W];
    for (int x = 0; x < k.W; ++x) {
        const Tap &t = tx[x];
        v[x] = bilerp(p0[t.i0], p0[t.i1], p1[t.i0], p1[t.i1], t.w0, t.w1, ty.w0, ty.w1);
    }
}

void norm_row(Call &k, int y, float *v, double *acc, double *sum) {
    const int W = k.W;
    std::fill(sum, sum + W, 0.0);
    int l = 0;
    long long first = 0;
    for (long long c0 = 0; c0 < k.C; c0 += BLOCK) {
        std::fill(acc, acc + W, 0.0);
        for (long long c = c0; c < std::min(k.C, c0 + BLOCK); ++c) {
            while (c >= first + k.layers[l].C) first += k.layers[l++].C;
            resize_row(k, l, (int)(c - first), y, v);
            for (int x = 0; x < W; ++x) acc[x] = square_acc(v[x], acc[x]);
        }
        for (int x = 0; x < W; ++x) sum[x] = sum[x] + acc[x];
    }
    for (int x = 0; x < W; ++x) k.n[(size_t)y * W + x] = norm_of(sum[x]);
}

// row y of the (normalised) map of layer l's channel c with its padding: p[0 .. W + 1] = columns -1 .. W
void padded_row(const Call &k, int l, int c, int y, float *v, float *p) {
    const int W = k.W;
    int ys;
    if (!pad(y, k.H, k.replicate, &ys)) {
        std::fill(p, p + W + 2, 0.0f);
        return;
    }
    resize_row(k, l, c, ys, v);
    if (k.norm)
        for (int x = 0; x < W; ++x) v[x] = normalised(v[x], k.n[(size_t)ys * W + x]);
    for (int xx = 0; xx < W + 2; ++xx) {
        int xs;
        p[xx] = pad(xx - 1, W, k.replicate, &xs) ? v[xs] : 0.0f;
    }
}

// One output row.  The three padded rows of a channel are formed here for every output row, so each source row is
// resized three times over the call: deliberate -- the rows stay independent (any thread, any order) and the
// twin is a yardstick, not a fast path.
template <typename Tout>
void pack_row(const Call &k, int y, float *v, float *rows) {
    const int W = k.W;
    const unsigned char *mk = k.marks ? k.marks + (size_t)y * W : nullptr;
    if (mk && !std::any_of(mk, mk + W, [](unsigned char m) { return m != 0; })) return;
    float *rm = rows, *r0 = rows + (W + 2), *rp = rows + 2 * (size_t)(W + 2);
    const size_t tstride = (size_t)(k.grad ? 3 : 1) * (size_t)k.cs;
    Tout *orow = (Tout *)k.out + (size_t)y * W * tstride;
    int l = 0;
    long long first = 0;
    for (long long c = k.c_begin; c < k.c_end; ++c) {
        while (c >= first + k.layers[l].C) first += k.layers[l++].C;
        const int cl = (int)(c - first);
        padded_row(k, l, cl, y, v, r0);
        if (k.grad) {
            padded_row(k, l, cl, y - 1, v, rm);
            padded_row(k, l, cl, y + 1, v, rp);
        }
        for (int x = 0; x < W; ++x) {
            if (mk && !mk[x]) continue;
            Tout *o = orow + (size_t)x * tstride + c;
            o[0] = (Tout)r0[x + 1];
            if (!k.grad) continue;
            const double sxm = col_sx(rm[x], r0[x], rp[x]), sym = col_sy(rm[x], rp[x]);
            const double sy0 = col_sy(rm[x + 1], rp[x + 1]);
            const double sxp = col_sx(rm[x + 2], r0[x + 2], rp[x + 2]), syp = col_sy(rm[x + 2], rp[x + 2]);
            o[k.cs] = (Tout)scaled(grad_x(sxm, sxp), k.sn);
            o[2 * (size_t)k.cs] = (Tout)scaled(grad_y(sym, sy0, syp), k.sn);
        }
    }
}

}  // namespace

extern "C" int fmpnp_hypercolumn_pack_cpu(const fmpnp_hc_layer *layers, int L, int B, int item, int H, int W,
                                          int flags, int c_begin, int c_end, int layout, int dtype_out, int cstride,
                                          int sobel_normalized, int sobel_replicate_pad, const unsigned char *marks,
                                          void *out, int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    long long C = 0;
    const int rc =
        check_pack_args(layers, L, B, item, H, W, flags, c_begin, c_end, layout, dtype_out, cstride, out, &C);
    if (rc) return rc;
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        Call k{layers, L, item, H, W, C, c_begin, c_end, cstride, (flags & FMPNP_HC_NORMALIZE) != 0,
               layout == FMPNP_LAYOUT_FGRAD, dtype_out == FMPNP_F64, sobel_normalized != 0, sobel_replicate_pad != 0,
               marks, out, {}, {}};
        k.tx.resize((size_t)L * (size_t)W);
        for (int l = 0; l < L; ++l) {
            const float sx = axis_scale(layers[l].W, W);
            for (int x = 0; x < W; ++x) k.tx[(size_t)l * (size_t)W + (size_t)x] = axis_tap(sx, layers[l].W, x);
        }
        if (k.norm) {
            k.n.resize((size_t)H * (size_t)W);
            const bool ok = fmpnp::host::deal(H, n_threads, [&]() {
                return [&k, v = std::vector<float>((size_t)W), acc = std::vector<double>((size_t)W),
                        sum = std::vector<double>((size_t)W)](long long y) mutable {
                    norm_row(k, (int)y, v.data(), acc.data(), sum.data());
                };
            });
            if (!ok) return FMPNP_ENOMEM;
        }
        const bool ok = fmpnp::host::deal(H, n_threads, [&]() {
            return [&k, v = std::vector<float>((size_t)W), rows = std::vector<float>(3 * ((size_t)W + 2))](long long y) mutable {
                if (k.f64) pack_row<double>(k, (int)y, v.data(), rows.data());
                else pack_row<float>(k, (int)y, v.data(), rows.data());
            };
        });
        if (!ok) return FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
    return 0;
}
