// fmpnp_hypercolumn_pack_impl.h -- the arithmetic of the fused hypercolumn pack beyond the assembly's own
// (fmpnp_hypercolumn_impl.h): the Sobel of the normalised map in the association the Sobel pack uses for fp32
// maps (csrc/fmpnp_pack.hip sb_row: column sums in fp64, then differences), the padding rule and the argument
// check.  The kernels of fmpnp_hypercolumn_pack.hip and the CPU twin of fmpnp_hypercolumn_pack_cpu.cpp both call
// these functions for every value they form; neither unit is compiled with contraction.  (sb_row itself is
// built with contraction allowed: its only products are by 2 and 0.125, which are exact, so a fused
// multiply-add there rounds as the separate operations here do.)
#pragma once
#include "fmpnp_hypercolumn_impl.h"

namespace fmpnp {
namespace hcp {

// column j of the 3 x 3 window, rows y - 1, y, y + 1 = a, d, g (widened fp32 values)
FMPNP_HC_HD double col_sx(double a, double d, double g) { return (a + 2.0 * d) + g; }
FMPNP_HC_HD double col_sy(double a, double g) { return g - a; }
// the gradients at the centre column from the sums of columns x - 1, x, x + 1
FMPNP_HC_HD double grad_x(double sxm, double sxp) { return sxp - sxm; }
FMPNP_HC_HD double grad_y(double sym, double sy0, double syp) { return (sym + 2.0 * sy0) + syp; }
// kornia's normalized=True divides by 8
FMPNP_HC_HD double scaled(double g, bool normalized) { return normalized ? g * 0.125 : g; }

// padding of the (normalised) map: coordinate i of an axis of n texels -> the texel read (replicate), or false
// for a zero (zero padding)
FMPNP_HC_HD bool pad(int i, int n, bool replicate, int *src) {
    if (i >= 0 && i < n) {
        *src = i;
        return true;
    }
    *src = i < 0 ? 0 : n - 1;
    return replicate;
}

// argument check of fmpnp_hypercolumn_pack* (host side): the layers and sizes as the assembly's, then the rest
inline int check_pack_args(const fmpnp_hc_layer *layers, int L, int B, int item, int H, int W, int flags, int c_begin,
                           int c_end, int layout, int dtype_out, int cstride, const void *out, long long *C_out) {
    if (flags & ~FMPNP_HC_NORMALIZE) return FMPNP_EINVAL;
    const float probe = 0.0f;  // (check_args wants a dense output; the packed one is checked below)
    const int rc = hc::check_args(layers, L, B, &probe, H, W, 0, 0, W, flags, C_out);
    if (rc) return rc;
    if (!out || item < 0 || item >= B) return FMPNP_EINVAL;
    if (c_begin < 0 || c_end <= c_begin || c_end > *C_out || cstride < *C_out) return FMPNP_EINVAL;
    if (layout != FMPNP_LAYOUT_FGRAD && layout != FMPNP_LAYOUT_F) return FMPNP_EINVAL;
    if (dtype_out != FMPNP_F32 && dtype_out != FMPNP_F64) return FMPNP_EINVAL;
    if (layout == FMPNP_LAYOUT_F && (dtype_out != FMPNP_F32 || cstride % 4)) return FMPNP_EINVAL;
    if ((uintptr_t)out % (dtype_out == FMPNP_F64 ? 8 : 4)) return FMPNP_EALIGN;
    if ((long long)H * W >= (1ll << 31)) return FMPNP_ETOOBIG;
    return 0;
}

}  // namespace hcp
}  // namespace fmpnp
