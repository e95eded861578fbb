// Precision "f16" (round 5): the implicit-GEMM tiles with ONE MFMA pass on fp16-rounded operands (NPASS = 1 of the kernel template in
// conv_f16x3_kernel.h) -- a labelled reduced-precision mode, never the default.  Register-staged tiles here, the LDS-DMA
// tiles in conv_f16x3_p1g.hip; translation units of their own so that all sets of instantiations compile side by side.
#include "conv_f16x3_kernel.h"

// `tile`: a register-staged tile t or its LDS-DMA form T_GLDS + t
int otvm_launch_tile_p1(int tile, Conv3Args& a, hipStream_t s, int S) {
    if (tile >= T_GLDS) return otvm_launch_glds_tile_p1(tile - T_GLDS, a, s, S);
    return launch_tile_form<false, 1, false>(tile, a, s, S);
}
