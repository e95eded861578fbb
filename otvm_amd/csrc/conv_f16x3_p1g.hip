// Precision "f16" (round 5): the LDS-DMA implicit-GEMM tiles with one MFMA pass (see conv_f16x3_p1.hip).
#include "conv_f16x3_kernel.h"

int otvm_launch_glds_tile_p1(int base, Conv3Args& a, hipStream_t s, int S) { return launch_tile_form<true, 1, false>(base, a, s, S); }
