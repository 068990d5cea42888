// fmpnp_hypercolumn_sparse_cpu.cpp -- fmpnp_hypercolumn_sparse_cpu: the CPU twin of fmpnp_hypercolumn_sparse
// with HOST pointers (include/fmpnp.h, "Sparse hypercolumns").
//
// The point's texel (locate) and every value (axis_tap, value_at, square_acc, norm_of, normalised) come from
// fmpnp_hypercolumn_impl.h, the header the kernel of fmpnp_hypercolumn_sparse.hip is built from; this unit is
// compiled without contraction and without -mfma, and the squares are summed in the contract's order (a chain
// per 64-channel block, the blocks ascending), so every row is the GPU's bit for bit.  The points are
// independent; they are dealt over the host threads.  An explicit CPU entry point, never a fallback.
#include <algorithm>
#include <atomic>
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
    const void *points;
    const int *item;
    int at;
    double p0, p1;
    void *out;
    bool f64;
    size_t ld;
    bool norm;
};

inline void put(const Call &k, size_t at, float v) {
    if (k.f64) ((double *)k.out)[at] = (double)v;
    else ((float *)k.out)[at] = v;
}

// row p; v: C floats of scratch.  False for an error row (written as zeros).
bool do_point(const Call &k, int p, float *v) {
    const size_t orow = (size_t)p * k.ld;
    int b, row, col;
    if (!locate(k.points, k.item, p, k.at, k.p0, k.p1, k.B, k.H, k.W, &b, &row, &col)) {
        for (long long c = 0; c < k.C; ++c) put(k, orow + (size_t)c, 0.0f);
        return false;
    }
    long long first = 0;
    for (int l = 0; l < k.L; ++l) {
        const fmpnp_hc_layer &ly = k.layers[l];
        const Tap ty = axis_tap(axis_scale(ly.H, k.H), ly.H, row), tx = axis_tap(axis_scale(ly.W, k.W), ly.W, col);
        for (int c = 0; c < ly.C; ++c) v[first + c] = value_at(ly, b, c, ty, tx);
        first += ly.C;
    }
    if (!k.norm) {
        for (long long c = 0; c < k.C; ++c) put(k, orow + (size_t)c, v[c]);
        return true;
    }
    double sum = 0.0;
    for (long long c0 = 0; c0 < k.C; c0 += BLOCK) {
        double acc = 0.0;
        for (long long c = c0; c < std::min(k.C, c0 + BLOCK); ++c) acc = square_acc(v[c], acc);
        sum = sum + acc;
    }
    const float n = norm_of(sum);
    for (long long c = 0; c < k.C; ++c) put(k, orow + (size_t)c, normalised(v[c], n));
    return true;
}

}  // namespace

extern "C" int fmpnp_hypercolumn_sparse_cpu(const fmpnp_hc_layer *layers, int L, int B, int H, int W,
                                            const void *points, const int *item, int N, int at, double p0, double p1,
                                            void *out, int dtype_out, long long ld_out, int flags, int *err_flag,
                                            int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    long long C = 0;
    const int rc = check_sparse_args(layers, L, B, H, W, points, N, at, p0, p1, out, dtype_out, ld_out, flags, &C);
    if (rc) return rc;
    if (N == 0) return 0;
    const Call k{layers, L, B, H, W, C, points, item, at, p0, p1, out, dtype_out == FMPNP_F64, (size_t)ld_out,
                 (flags & FMPNP_HC_NORMALIZE) != 0};
    std::atomic<int> bad(0);
    // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
    const bool ok = fmpnp::host::deal(N, n_threads, [&]() {
        return [&k, &bad, v = std::vector<float>((size_t)C)](long long p) mutable {
            if (!do_point(k, (int)p, v.data())) bad = 1;
        };
    });
    if (!ok) return FMPNP_ENOMEM;
    if (bad && err_flag) *err_flag |= 1;
    return bad ? FMPNP_ERANGE : 0;
}
