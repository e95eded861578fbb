// Index and weight arithmetic of the patch conv's upsampled source (conv_patch_f16x3.hip, otvm_conv2d_up): one axis of the 2x
// bilinear upsampling (align_corners = False) as upsample_bilinear_kernel / upsample2x_bilinear_kernel (resample.hip) compute it,
// plus the place of the two source samples inside the tile's source patch in LDS.  Host and device: tests/test_upfold_index_cpu.py
// compiles it into a host program and walks every coordinate of every tile.
#pragma once

#if defined(__HIPCC__)
#define OTVM_UPFOLD_HD __host__ __device__ inline
#else
#define OTVM_UPFOLD_HD inline
#endif

struct OtvmUpAxis {
    int i0, i1;      // source indices, inside [0, n)
    float l;         // weight of i1 (1 - l: weight of i0): 0, 0.25 or 0.75 inside the image
    int s0, s1;      // rows / columns of i0, i1 in the tile's source patch, inside [0, ns)
    int code;        // l = 0.25f * code for every coordinate inside the image (0, 1, 3)
};

// first source row / column a tile needs whose first fine row / column is t0 (even): the halo pixel t0 - 1 reads t0 / 2 - 1
OTVM_UPFOLD_HD int otvm_upfold_origin(int t0) { return (t0 >> 1) - 1; }
// source rows / columns a tile of `t` fine rows / columns (even) reads, halo included
constexpr int otvm_upfold_extent(int t) { return t / 2 + 2; }

// o: fine coordinate -- any integer: the conv's padding lies outside [0, 2 n), its values are never used but its indices and
// slots stay in range; n: source extent; org = otvm_upfold_origin(tile's first fine coordinate); ns: extent of the source patch
OTVM_UPFOLD_HD OtvmUpAxis otvm_upfold_axis(int o, int n, int org, int ns) {
#pragma clang fp contract(off)
    OtvmUpAxis a;
    float f = ((float)o + 0.5f) * 0.5f - 0.5f;
    f = f < 0.f ? 0.f : f;
    const int fi = (int)f;
    a.l = f - (float)fi;
    a.i0 = fi > n - 1 ? n - 1 : fi;                       // (fi <= n - 1 inside the image)
    a.i1 = a.i0 + (a.i0 < n - 1 ? 1 : 0);
    const int r0 = a.i0 - org, r1 = a.i1 - org;
    a.s0 = r0 < 0 ? 0 : (r0 > ns - 1 ? ns - 1 : r0);      // (no clamp acts inside the image)
    a.s1 = r1 < 0 ? 0 : (r1 > ns - 1 ? ns - 1 : r1);
    a.code = o <= 0 ? 0 : ((o & 1) ? 1 : 3);
    return a;
}
