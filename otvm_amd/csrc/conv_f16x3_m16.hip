// The LDS-DMA implicit-GEMM f16x3 tiles on v_mfma_f32_16x16x32_f16 (round 5, "M16": the kernel, its comment and the tile table live
// in conv_f16x3_kernel.h, the dispatch in conv_f16x3.hip).  A translation unit of its own: the instantiations compile beside the others.
#include "conv_f16x3_kernel.h"

int otvm_launch_m16_tile(int base, Conv3Args& a, hipStream_t s, int S) { return launch_tile_form<true, 3, true>(base, a, s, S); }
