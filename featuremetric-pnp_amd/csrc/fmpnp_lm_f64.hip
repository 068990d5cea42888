// fmpnp_lm_f64.hip -- LM kernel variants for double texels (see fmpnp_lm_impl.h).  One
// translation unit per storage type, so the variants compile in parallel.
#include "fmpnp_lm_impl.h"

namespace fmpnp {

const void *lm_kernel_ptr_f64(int wps, bool team, bool ratio, int var) { return lm_pick<double>(wps, team, ratio, var); }

}  // namespace fmpnp
