// fmpnp_lm_f16.hip -- LM kernel variants for binary16 texels (FMPNP_F16; see fmpnp_lm_impl.h).  One
// translation unit per storage type, so the variants compile in parallel.  Texels and descriptors are
// widened exactly to fp64 by the gather ((double) of a _Float16: v_cvt_f32_f16, v_cvt_f64_f32); a lane's
// 16-byte load holds V = 8 channels, so one trip of two rounds covers 512 channels and the four-round
// chunk 1024.  Nearest sampling of the packed f, gx, gy planes only: the bilinear and f-only variants are
// not instantiated (validated away by the planner, include/fmpnp.h).
#include "fmpnp_lm_impl.h"

namespace fmpnp {

typedef void (*LmFn)(LaunchArgs);
template <int WPS, bool TEAM, bool RATIO>
static LmFn pick_var(int var) {
    if (var == VAR_GM) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_GM>;
    if (var == VAR_NEAREST) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_NEAREST>;
    if (var == VAR_GM_SPEC || var == VAR_NEAREST_SPEC || var == VAR_GM_SPEC_H || var == VAR_NEAREST_SPEC_H) {
        if constexpr (WPS == WPS_LATENCY && !TEAM) {  // speculation (+ helpers): latency build, G = 1
            if (var == VAR_GM_SPEC) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_GM_SPEC>;
            if (var == VAR_NEAREST_SPEC) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_NEAREST_SPEC>;
            if (var == VAR_GM_SPEC_H) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_GM_SPEC_H>;
            return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_NEAREST_SPEC_H>;
        }
        return nullptr;
    }
    if (var == VAR_GM_H || var == VAR_NEAREST_H) {  // first-evaluation helpers without speculation
        if constexpr (WPS == WPS_LATENCY && !TEAM) {
            if (var == VAR_GM_H) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_GM_H>;
            return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_NEAREST_H>;
        }
        return nullptr;
    }
    if (var == VAR_GM_W || var == VAR_NEAREST_W) {  // packed windows (fmpnp_feature_pnp): latency build
        if constexpr (WPS == WPS_LATENCY) {
            if (var == VAR_GM_W) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_GM_W>;
            return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_NEAREST_W>;
        }
        return nullptr;
    }
    if (var == VAR_GM_H_W || var == VAR_NEAREST_H_W) {  // ... with the first-evaluation helpers
        if constexpr (WPS == WPS_LATENCY && !TEAM) {
            if (var == VAR_GM_H_W) return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_GM_H_W>;
            return lm_kernel<_Float16, WPS, TEAM, RATIO, VAR_NEAREST_H_W>;
        }
        return nullptr;
    }
    // the _512 carve (fp32 texels only), bilinear sampling and FMPNP_LAYOUT_F (validated: FMPNP_EINVAL)
    return nullptr;
}
template <int WPS>
static LmFn pick(bool team, bool ratio, int var) {
    if (team) return ratio ? pick_var<WPS, true, true>(var) : pick_var<WPS, true, false>(var);
    return ratio ? pick_var<WPS, false, true>(var) : pick_var<WPS, false, false>(var);
}

const void *lm_kernel_ptr_f16(int wps, bool team, bool ratio, int var) {
    if (wps == WPS_WIDE) return nullptr;  // the bilinear cell memo only
    // the 128-VGPR throughput build is only planned with G == 1
    if (wps == WPS_THROUGHPUT) return (const void *)(ratio ? pick_var<WPS_THROUGHPUT, false, true>(var)
                                                           : pick_var<WPS_THROUGHPUT, false, false>(var));
    return (const void *)pick<WPS_LATENCY>(team, ratio, var);
}

}  // namespace fmpnp
