// fmpnp_dense_impl.h -- what the dense-feature unit's kernels (fmpnp_dense.hip) and their CPU twins
// (fmpnp_dense_cpu.cpp) share beyond the encoder's and the assembly's own headers: the pyramid step's value and
// divisor, and the argument checks (include/fmpnp.h, "dense features", states the contract).  Plain C++ (the twin is
// built by the host compiler), __host__ __device__ under hipcc; neither unit is compiled with contraction.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fmpnp.h"
#include "fmpnp_encoder_impl.h"
#include "fmpnp_hypercolumn_impl.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fmpnp {
namespace dense {

// what the norm divides by: F.normalize's clamp max(n, 1e-12f); a NaN norm stays NaN
FMPNP_HC_HD float divisor(float n) { return n < 1e-12f ? 1e-12f : n; }

// the step's value before the division: cur, or cur plus the resized prev in one fp32 add
FMPNP_HC_HD float summed(float cur, float resized) { return cur + resized; }

// argument check of fmpnp_dense_pyramid_step* (host side)
inline int step_args(const void *cur, const void *prev, int B, int C, int h, int w, int hp, int wp, const void *out,
                     int flags) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || !cur || !out) return FMPNP_EINVAL;
    if (flags & ~FMPNP_PYR_NORMALIZE) return FMPNP_EINVAL;
    if (prev && (hp < 1 || wp < 1)) return FMPNP_EINVAL;
    if (h > hc::MAX_SIZE || w > hc::MAX_SIZE || B > hc::MAX_SIZE || C > hc::MAX_SIZE) return FMPNP_ETOOBIG;
    if (prev && (hp > hc::MAX_SIZE || wp > hc::MAX_SIZE)) return FMPNP_ETOOBIG;
    // (each factor is at most 2^24 and the running product is below 2^31 once checked: no size_t overflow)
    const size_t bc = (size_t)B * (size_t)C;
    if (bc >= enc::MAX_ELEMS || bc * (size_t)h >= enc::MAX_ELEMS || bc * (size_t)h * (size_t)w >= enc::MAX_ELEMS)
        return FMPNP_ETOOBIG;
    if (prev && (bc * (size_t)hp >= enc::MAX_ELEMS || bc * (size_t)hp * (size_t)wp >= enc::MAX_ELEMS))
        return FMPNP_ETOOBIG;
    return 0;
}

}  // namespace dense
}  // namespace fmpnp
