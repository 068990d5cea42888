// Host listing of the LM kernel picker (lm_kernel_ptr): for every storage type x build x team x ratio x
// variant code, one line with the arguments and the symbol of the kernel handed back (dladdr), or null.
// It needs no device.  Built by the Makefile with -rdynamic against the four LM units' objects, run by
// tests/test_lm_picker.py (CPU), which compares the listing with tests/golden/lm_picker.txt.
#include <dlfcn.h>
#include <stdio.h>

#include "fmpnp_internal.h"

int main() {
    const int dtypes[3] = {FMPNP_F32, FMPNP_F64, FMPNP_F16};
    const char *const dtype_names[3] = {"f32", "f64", "f16"};
    const int builds[3] = {FMPNP_BUILD_WIDE, FMPNP_BUILD_LATENCY, FMPNP_BUILD_THROUGHPUT};
    const char *const build_names[3] = {"wide", "latency", "throughput"};
    for (int d = 0; d < 3; ++d)
        for (int b = 0; b < 3; ++b)
            for (int team = 0; team < 2; ++team) {
                if (builds[b] == FMPNP_BUILD_THROUGHPUT && team) continue;  // never planned
                for (int ratio = 0; ratio < 2; ++ratio)
                    for (int var = 0; var <= FMPNP_VAR_NEAREST_H_W; ++var) {
                        const void *f = fmpnp::lm_kernel_ptr(dtypes[d], builds[b], team != 0, ratio != 0, var);
                        Dl_info info;
                        const char *name = "null";
                        if (f) name = dladdr(f, &info) && info.dli_sname ? info.dli_sname : "?";
                        printf("%s %s team=%d ratio=%d var=%d %s\n", dtype_names[d], build_names[b], team, ratio, var, name);
                    }
            }
    return 0;
}
