// fmpnp_lm_f16.hip -- LM kernel variants for binary16 texels (FMPNP_F16; see fmpnp_lm_impl.h).  One
// translation unit per storage type, so the variants compile in parallel.  Texels and descriptors are
// widened exactly to fp64 by the gather ((double) of a _Float16: v_cvt_f32_f16, v_cvt_f64_f32); a lane's
// 16-byte load holds V = 8 channels, so one trip of two rounds covers 512 channels and the four-round
// chunk 1024.  Nearest sampling of the packed f, gx, gy planes only: the bilinear and f-only variants are
// not instantiated (fmpnp_internal.h lm_built; validated away by the planner, include/fmpnp.h).
#include "fmpnp_lm_impl.h"

namespace fmpnp {

const void *lm_kernel_ptr_f16(int wps, bool team, bool ratio, int var) { return lm_pick<_Float16>(wps, team, ratio, var); }

}  // namespace fmpnp
