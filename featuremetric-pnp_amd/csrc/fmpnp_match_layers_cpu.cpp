// fmpnp_match_layers_cpu.cpp -- fmpnp_exhaustive_match_layers_cpu: the CPU twin of fmpnp_exhaustive_match_layers
// (include/fmpnp.h, "layered matching") with HOST pointers.
//
// The contract restated for a CPU core.  The coarse scores of a row are the fmaf chains of fmpnp_host.h over each
// layer's own channels (what the exact-fp32 MFMA computes per score); a score is formed from them by taps_at,
// resized and summed of fmpnp_match_layers_impl.h, the code combine_kernel runs; the norm plane is the assembly twin's pass 1
// (fp64 chains per 64-channel block of the concatenated index, partials in ascending order, (float)sqrt) from
// fmpnp_hypercolumn_impl.h; the row reduction is select_row of fmpnp_host.h.  The unit is built without
// contraction and without -mfma, so scores, argmax, d1, d_k and mask are the GPU's bit for bit.  An explicit CPU
// entry point -- a parity bridge and a baseline -- never a fallback of the HIP entry points.
#include <algorithm>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_match_layers_impl.h"

namespace {

using namespace fmpnp::hc;
using fmpnp::ml::Taps;

constexpr int JB = 1024;  // columns per accumulator block of the chains (stays in L1)

// row y of the norm plane: n[x] for x in [0, W); tx: every layer's taps along x ([L][W])
void norm_row(const fmpnp_hc_layer *layers, int L, int item, int H, int W, long long C, int y, const Tap *tx,
              double *acc, double *sum, float *n) {
    std::fill(sum, sum + W, 0.0);
    int l = 0;
    long long first = 0;  // layer l's first concatenated channel
    Tap ty = axis_tap(axis_scale(layers[0].H, H), layers[0].H, y);
    for (long long c0 = 0; c0 < C; c0 += BLOCK) {
        std::fill(acc, acc + W, 0.0);
        for (long long c = c0, end = std::min(C, c0 + BLOCK); c < end; ++c) {
            while (c >= first + layers[l].C) {
                first += layers[l].C;
                ++l;
                ty = axis_tap(axis_scale(layers[l].H, H), layers[l].H, y);
            }
            const fmpnp_hc_layer &ly = layers[l];
            const float *plane = ly.data + (size_t)item * (size_t)ly.stride_b + (size_t)(c - first) * (size_t)ly.stride_c;
            const float *p0 = plane + (size_t)ty.i0 * (size_t)ly.stride_y, *p1 = plane + (size_t)ty.i1 * (size_t)ly.stride_y;
            const Tap *t = tx + (size_t)l * (size_t)W;
            for (int x = 0; x < W; ++x) {
                const float v = bilerp(p0[t[x].i0], p0[t[x].i1], p1[t[x].i0], p1[t[x].i1], t[x].w0, t[x].w1, ty.w0, ty.w1);
                acc[x] = square_acc(v, acc[x]);
            }
        }
        for (int x = 0; x < W; ++x) sum[x] = sum[x] + acc[x];
    }
    for (int x = 0; x < W; ++x) n[x] = norm_of(sum[x]);
}

}  // namespace

extern "C" int fmpnp_exhaustive_match_layers_cpu(const float *sparse, int N, int ld_sparse, const fmpnp_hc_layer *layers,
                                                 int L, int B, int item, int H, int W, int flags, int top_k, double ratio,
                                                 int *argmax, float *top, float *kth, unsigned char *mask, float *scores,
                                                 int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    long long C = 0, coarse_floats = 0;
    const int rc = fmpnp::ml::check_args(sparse, N, ld_sparse, layers, L, B, item, H, W, flags, &C, &coarse_floats);
    if (rc) return rc;
    const int WH = H * W;
    if (top_k < 1 || top_k > WH || !(ratio == ratio)) return FMPNP_EINVAL;
    if (N == 0) return 0;
    if (!argmax || !top || !kth || !mask) return FMPNP_EINVAL;
    const bool norm = (flags & FMPNP_HC_NORMALIZE) != 0;
    const float ratio2 = (float)(ratio * ratio);
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        // the taps and weights depend on (layer, texel) only: set up once, for every row
        std::vector<Taps> taps((size_t)L * (size_t)WH);
        for (int l = 0; l < L; ++l)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    taps[(size_t)l * WH + (size_t)y * W + x] = fmpnp::ml::taps_at(layers[l].H, layers[l].W, H, W, y, x);
        std::vector<float> n;
        if (norm) {  // the norm plane, once per call
            n.resize((size_t)WH);
            std::vector<Tap> tx((size_t)L * (size_t)W);
            for (int l = 0; l < L; ++l) {
                const float sx = axis_scale(layers[l].W, W);
                for (int x = 0; x < W; ++x) tx[(size_t)l * W + x] = axis_tap(sx, layers[l].W, x);
            }
            const bool ok = fmpnp::host::deal(H, n_threads, [&]() {
                return [&, acc = std::vector<double>((size_t)W), sum = std::vector<double>((size_t)W)](long long y) mutable {
                    norm_row(layers, L, item, H, W, C, (int)y, tx.data(), acc.data(), sum.data(), n.data() + (size_t)y * W);
                };
            });
            if (!ok) return FMPNP_ENOMEM;
        }
        const float *nn = norm ? n.data() : nullptr;
        const Taps *tp = taps.data();
        const bool ok = fmpnp::host::deal(N, n_threads, [&]() {
            return [=, coarse = std::vector<float>((size_t)coarse_floats), rowbuf = std::vector<float>(scores ? 0 : (size_t)WH),
                    keys = std::vector<unsigned>((size_t)WH)](long long i) mutable {
                // S_l[i]: one fmaf chain per coarse texel over the layer's own channels, ascending
                const float *d = sparse + (size_t)i * (size_t)ld_sparse;
                float *s = coarse.data();
                for (int l = 0; l < L; ++l) {
                    const fmpnp_hc_layer &ly = layers[l];
                    const int wh = ly.H * ly.W;
                    const float *dense = ly.data + (size_t)item * (size_t)ly.stride_b;
                    for (int j0 = 0; j0 < wh; j0 += JB)
                        fmpnp::host::fmaf_chains(d, dense + j0, (size_t)ly.stride_c, ly.C, std::min(JB, wh - j0), s + j0);
                    d += ly.C;
                    s += wh;
                }
                // the resizes, the ascending sum and the division
                float *row = scores ? scores + (size_t)i * (size_t)WH : rowbuf.data();
                for (int p = 0; p < WH; ++p) {
                    float t = 0.f;
                    const float *m = coarse.data();
                    for (int l = 0; l < L; ++l) {
                        t = fmpnp::ml::summed(t, fmpnp::ml::resized(m, tp[(size_t)l * WH + p]), l == 0);
                        m += layers[l].H * layers[l].W;
                    }
                    row[p] = nn ? normalised(t, nn[p]) : t;
                }
                fmpnp::host::select_row(row, WH, top_k, ratio2, keys.data(), argmax + i, top + i, kth + i, mask + i);
            };
        });
        return ok ? 0 : FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}
