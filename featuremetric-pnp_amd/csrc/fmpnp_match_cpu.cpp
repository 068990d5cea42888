// fmpnp_match_cpu.cpp -- fmpnp_exhaustive_match_cpu: the CPU twin of fmpnp_exhaustive_match
// (s2dhm/pose_prediction/exhaustive_search.py:8-55) with HOST pointers.
//
// The contract of fmpnp_match.hip restated for a CPU core: every score is one fp32 fmaf chain over
// k = 0 .. C-1 in ascending order from +0 (what v_mfma_f32_32x32x2_f32 computes), the argmax takes the
// lowest flat index among equal maxima with NaN above everything, d_k is the exact top_k-th largest
// value under the same order-preserving key, and the mask is one fp32 product against d_k.  So the
// scores, argmax, d1, d_k and mask are the GPU's bit for bit.  An explicit CPU entry point -- a parity
// bridge and a baseline -- never a fallback of the HIP entry points.
//
// fmaf must be the correctly rounded fused operation whatever the host: the unit is built without
// contraction and without -mfma, so std::fmaf is libm's (correctly rounded in software where the core
// has no FMA); where the core has FMA the same loop compiled for it runs instead (one vfmadd per
// product: the same value).
//
// fmpnp_exhaustive_match_ex_cpu adds the REFERENCE of the opt-in fp16 precision (FMPNP_MATCH_F16): operands
// rounded to binary16, exact products accumulated in fp64 in ascending k, one rounding to fp32, then the same
// key, select and mask.  It is not a twin: the order inside the GPU's fp16 MFMA is not documented, and the GPU's
// f16 scores lie within a bound of these (include/fmpnp.h, "fp16 precision"), not on them.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"

namespace {

constexpr int JB = 1024;  // columns per accumulator block (stays in L1)

// ---- the reference of the fp16 precision (FMPNP_MATCH_F16, include/fmpnp.h "fp16 precision") ----
using fmpnp::host::fl16;  // (fmpnp_host.h: binary16, round-to-nearest-even, as an fp32 value)

// acc64[j] += (double)a[k] * dense16[k][j] for k ascending (the operands already rounded, every product exact
// in fp64), then one rounding to fp32
void row_block_f16(const float *a, const float *dense, size_t ld_dense, int C, int nj, float *out) {
    double acc[JB];
    for (int j = 0; j < nj; ++j) acc[j] = 0.0;
    for (int k = 0; k < C; ++k) {
        const double ak = (double)a[k];
        const float *d = dense + (size_t)k * ld_dense;
        for (int j = 0; j < nj; ++j) acc[j] += ak * (double)d[j];
    }
    for (int j = 0; j < nj; ++j) out[j] = (float)acc[j];
}

// (the key of fmpnp_match.hip, the select and the mask: fmpnp_host.h select_row, shared with the layered twin)

int match_cpu(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense, int top_k,
              double ratio, int *argmax, float *top, float *kth, unsigned char *mask, float *scores, int n_threads,
              int precision) {
    if (precision != FMPNP_MATCH_F32 && precision != FMPNP_MATCH_F16) return FMPNP_EINVAL;
    if (N < 0 || C <= 0 || WH <= 0 || ld_sparse < C || ld_dense < WH || n_threads < 0) return FMPNP_EINVAL;
    if (top_k < 1 || top_k > WH || !(ratio == ratio)) return FMPNP_EINVAL;
    if (N == 0) return 0;
    if (!sparse || !dense || !argmax || !top || !kth || !mask) return FMPNP_EINVAL;
    // a row's scores: the fmaf chains over k ascending (fmpnp_host.h), or the f16 reference's below
    fmpnp::host::fmaf_chains_fn row_block = fmpnp::host::fmaf_chains;
    std::vector<float> sparse16, dense16;  // the f16 reference's operands, rounded once
    if (precision == FMPNP_MATCH_F16) {
        try {
            sparse16.resize((size_t)N * C);
            dense16.resize((size_t)C * WH);
        } catch (...) {
            return FMPNP_ENOMEM;
        }
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < C; ++k) sparse16[(size_t)i * C + k] = fl16(sparse[(size_t)i * ld_sparse + k]);
        for (int k = 0; k < C; ++k)
            for (int j = 0; j < WH; ++j) dense16[(size_t)k * WH + j] = fl16(dense[(size_t)k * ld_dense + j]);
        sparse = sparse16.data(), ld_sparse = C;
        dense = dense16.data(), ld_dense = WH;
        row_block = row_block_f16;
    }
    const float ratio2 = (float)(ratio * ratio);
    // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
    const bool ok = fmpnp::host::deal(N, n_threads, [&]() {
        return [=, rowbuf = std::vector<float>(scores ? 0 : (size_t)WH), keys = std::vector<unsigned>((size_t)WH)](
                   long long i) mutable {
            float *row = scores ? scores + (size_t)i * WH : rowbuf.data();
            for (int j0 = 0; j0 < WH; j0 += JB)
                row_block(sparse + (size_t)i * ld_sparse, dense + j0, (size_t)ld_dense, C, std::min(JB, WH - j0),
                          row + j0);
            fmpnp::host::select_row(row, WH, top_k, ratio2, keys.data(), argmax + i, top + i, kth + i, mask + i);
        };
    });
    return ok ? 0 : FMPNP_ENOMEM;
}

}  // namespace

extern "C" int fmpnp_exhaustive_match_cpu(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                          int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                          unsigned char *mask, float *scores, int n_threads) {
    return match_cpu(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask, scores, n_threads,
                     FMPNP_MATCH_F32);
}

extern "C" int fmpnp_exhaustive_match_ex_cpu(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH,
                                             int ld_dense, int top_k, double ratio, int *argmax, float *top, float *kth,
                                             unsigned char *mask, float *scores, int n_threads, int precision) {
    return match_cpu(sparse, N, ld_sparse, dense, C, WH, ld_dense, top_k, ratio, argmax, top, kth, mask, scores, n_threads,
                     precision);
}
