// The implicit-GEMM f16x3 tiles with LDS-DMA weight stages (round 5; the kernel, its long comment and the tile table live in
// conv_f16x3_kernel.h, the dispatch in conv_f16x3.hip).  A translation unit of its own so that the sets of tile instantiations
// compile side by side.
#include "conv_f16x3_kernel.h"

int otvm_launch_glds_tile(int base, Conv3Args& a, hipStream_t s, int S) { return launch_tile_form<true, 3, false>(base, a, s, S); }
