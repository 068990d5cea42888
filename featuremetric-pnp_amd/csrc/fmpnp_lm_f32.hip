// fmpnp_lm_f32.hip -- LM kernel variants for float texels (see fmpnp_lm_impl.h).  One
// translation unit per storage type, so the variants compile in parallel.
#include "fmpnp_lm_impl.h"

namespace fmpnp {

const void *lm_kernel_ptr_f32(int wps, bool team, bool ratio, int var) { return lm_pick<float>(wps, team, ratio, var); }

}  // namespace fmpnp
