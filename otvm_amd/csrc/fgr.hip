// Foreground outputs of a frame (include/otvm_hip.h: otvm_fgr_outputs): crop the padded alpha and F planes, quantise to RGBA,
// composite over a new background -- one pass, every input read once.  HBM-bound: at 1920x1080 33 MB read (alpha + three F planes)
// + 6 MB of background, 8 + 6 MB of bytes (+ 25 MB for the fp32 F) written.  Compiled with -ffp-contract=off: tests/fgr_ref.py
// restates the arithmetic operation by operation and the outputs are compared bit for bit.
//
// A thread takes four consecutive pixels of one output row.  When the width is a multiple of four (and the bases are 16-byte
// aligned) every group starts 16 / 12 / 16 bytes into its RGBA / RGB / fp32 rows' own alignment: one 16-byte store, three dwords,
// one 16-byte store per plane.  Otherwise a row's groups start at any byte: the same values go out pixel by pixel (one dword per
// RGBA pixel, bytes for RGB), as the last one to three pixels of a row always do.  The padded planes are read with dword loads
// (the left padding puts the rows at any dword); consecutive lanes read consecutive 16-byte pieces.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }      // false for NaN and +-inf

// (uint8) trunc(v * 255): the reference's (x * 255).byte() (eval.py:209) made total -- clamped to the byte range; non-finite = 0
__device__ __forceinline__ unsigned quant_u8(float v, bool ok) {
    const float t = fminf(fmaxf(truncf(v * 255.f), 0.f), 255.f);
    return (ok && finite_f(v)) ? (unsigned)(int)t : 0u;
}

__global__ __launch_bounds__(256) void fgr_outputs_kernel(const otvm_fgr_params p, const int vec) {
    const int n4 = (p.W + 3) >> 2;
    const int64_t total = (int64_t)p.H * n4, P = (int64_t)p.Hp * p.Wp, N = (int64_t)p.H * p.W;
    const float s = 1.f / 255.f;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.W - x0 < 4 ? p.W - x0 : 4;
        const int64_t ip = (int64_t)(y + p.lh) * p.Wp + (x0 + p.lw), o = (int64_t)y * p.W + x0;
        float a[4], F[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = k < n;
            a[k] = (in && p.alpha_p) ? p.alpha_p[ip + k] : 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) F[c][k] = in ? p.fgr_p[c * P + ip + k] : 0.f;
        }
        const bool full = n == 4 && vec;
        if (p.fgr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (full) {
                    *reinterpret_cast<f32x4*>(p.fgr + c * N + o) = f32x4{F[c][0], F[c][1], F[c][2], F[c][3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) p.fgr[c * N + o + k] = F[c][k];
                }
            }
        }
        if (p.rgba_u8) {
            unsigned px[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                px[k] = quant_u8(a[k], true) << 24;
#pragma unroll
                for (int j = 0; j < 3; ++j) px[k] |= quant_u8(F[p.u8_rgb ? j : 2 - j][k], true) << (8 * j);
            }
            unsigned* dst = reinterpret_cast<unsigned*>(p.rgba_u8) + o;
            if (full) {
                *reinterpret_cast<u32x4*>(dst) = u32x4{px[0], px[1], px[2], px[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) dst[k] = px[k];
            }
        }
        if (p.comp_u8) {
            unsigned by[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const unsigned bgb = p.bg_u8 ? (k < n ? (unsigned)p.bg_u8[(o + k) * 3 + j] : 0u) : (unsigned)p.bg_color[j];
                    const float f = F[p.u8_rgb ? j : 2 - j][k];
                    const float bgf = (float)bgb * s;
                    const float c = (f * a[k]) + (bgf * (1.f - a[k]));
                    by[k * 3 + j] = quant_u8(c, finite_f(f) && finite_f(a[k]));
                }
            }
            if (full) {
                unsigned* dst = reinterpret_cast<unsigned*>(p.comp_u8 + o * 3);
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    dst[d] = by[4 * d] | (by[4 * d + 1] << 8) | (by[4 * d + 2] << 16) | (by[4 * d + 3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) p.comp_u8[(o + k) * 3 + j] = (unsigned char)by[k * 3 + j];
                    }
            }
        }
    }
}

}  // namespace

extern "C" int otvm_fgr_outputs(const otvm_fgr_params* p, void* stream) {
    OTVM_REQUIRE(p && p->fgr_p, "otvm_fgr_outputs: null parameters / F planes");
    OTVM_REQUIRE(p->fgr || p->rgba_u8 || p->comp_u8, "otvm_fgr_outputs: no output requested");
    OTVM_REQUIRE(p->alpha_p || !(p->rgba_u8 || p->comp_u8), "otvm_fgr_outputs: rgba_u8 / comp_u8 need the padded alpha plane");
    OTVM_REQUIRE(p->H > 0 && p->W > 0 && p->lh >= 0 && p->lw >= 0 && p->H + p->lh <= p->Hp && p->W + p->lw <= p->Wp,
                 "otvm_fgr_outputs: a %dx%d output at (%d, %d) does not lie inside the %dx%d padded frame", p->W, p->H, p->lw, p->lh,
                 p->Wp, p->Hp);
    OTVM_REQUIRE((((uintptr_t)p->alpha_p | (uintptr_t)p->fgr_p | (uintptr_t)p->fgr | (uintptr_t)p->rgba_u8) & 3) == 0,
                 "otvm_fgr_outputs: alpha_p / fgr_p / fgr / rgba_u8 must be 4-byte aligned");
    const int vec = (p->W & 3) == 0 && (((uintptr_t)p->fgr | (uintptr_t)p->rgba_u8) & 15) == 0 && ((uintptr_t)p->comp_u8 & 3) == 0;
    const int64_t total = (int64_t)p->H * ((p->W + 3) / 4);
    const int64_t b = (total + 255) / 256;
    hipLaunchKernelGGL(fgr_outputs_kernel, dim3((unsigned)(b > 16384 ? 16384 : b)), dim3(256), 0, (hipStream_t)stream, *p, vec);
    OTVM_CHECK_LAUNCH("otvm_fgr_outputs");
    return 0;
}
