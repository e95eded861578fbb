// Working-resolution matting (include/otvm_hip.h: otvm_downsample_*, otvm_guided_coeffs, otvm_guided_apply): the network runs
// on an s x s block mean of the frame (s = 2, 3, 4) and its alpha / F planes come back to the frame's own resolution through
// the colour-guide fast guided filter (He & Sun).  Compiled with -ffp-contract=off: tests/guided_ref.py restates every step
// and the outputs are compared bit for bit.
//
//   reductions   : integer arithmetic, one thread per working pixel.
//   coefficients : the targets are quantised to 16 bits once, so every window sum is an exact 32-bit integer (81 * 255 * 65535
//                  < 2^31) and order-free: a workgroup stages its 32x8 tile plus the r halo in LDS (guide bytes packed in a dword,
//                  targets as 16-bit integers) and every thread sums its clipped window from there -- no atomics.  The 3x3 solve
//                  (adjugate) runs in fp64 from the exact integer numerators; (a0, a1, a2, b) leaves as fp32.
//   box mean     : fp64, rows in ascending x into LDS, then columns in ascending y, / N, rounded to fp32.
//   apply        : the hot pass, HBM-bound.  A thread takes four consecutive pixels of a full-resolution row (as fgr.hip does):
//                  12 guide bytes in, bilinear lookup of the mean coefficients (L2-resident: 1 / s^2 of the output), 16-byte
//                  stores of the fp32 planes and one dword of alpha bytes when the width is a multiple of four.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TX = 32, TY = 8, RMAX = 4;
constexpr int TILE_MAX = (TX + 2 * RMAX) * (TY + 2 * RMAX);

static inline unsigned grid_1d(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------------------------------------ reductions
__global__ __launch_bounds__(256) void downsample_u8_kernel(const uint8_t* __restrict__ src, int H, int W, int s, int h, int w,
                                                            uint8_t* __restrict__ dst) {
    const int64_t total = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const int y0 = y * s, x0 = x * s, y1 = min(y0 + s, H), x1 = min(x0 + s, W);
        const int n = (y1 - y0) * (x1 - x0);                    // >= 1: h = ceil(H / s), w = ceil(W / s)
        int sum0 = 0, sum1 = 0, sum2 = 0;
        for (int yy = y0; yy < y1; ++yy) {
            const uint8_t* row = src + ((int64_t)yy * W + x0) * 3;
            for (int k = 0; k < x1 - x0; ++k) {
                sum0 += row[k * 3];
                sum1 += row[k * 3 + 1];
                sum2 += row[k * 3 + 2];
            }
        }
        dst[i * 3] = (uint8_t)((sum0 + n / 2) / n);
        dst[i * 3 + 1] = (uint8_t)((sum1 + n / 2) / n);
        dst[i * 3 + 2] = (uint8_t)((sum2 + n / 2) / n);
    }
}

// conservative: a block is fg (bg) only when every pixel of it is exactly fg (bg); the unknown band never shrinks
__global__ __launch_bounds__(256) void downsample_trimap_kernel(const float* __restrict__ src, int H, int W, int s, int h, int w,
                                                                float* __restrict__ dst) {
    const int64_t total = (int64_t)h * w, P = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const int y0 = y * s, x0 = x * s, y1 = min(y0 + s, H), x1 = min(x0 + s, W);
        bool all_bg = true, all_fg = true;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) {
                const int64_t j = (int64_t)yy * W + xx;
                all_bg = all_bg && src[j] == 1.f;
                all_fg = all_fg && src[2 * P + j] == 1.f;
            }
        const bool fg = all_fg && !all_bg, bg = all_bg && !all_fg;     // (both: not a one-hot input -- unknown)
        dst[i] = bg ? 1.f : 0.f;
        dst[total + i] = (fg || bg) ? 0.f : 1.f;
        dst[2 * total + i] = fg ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void downsample_labels_kernel(const uint8_t* __restrict__ src, int H, int W, int s, int h, int w,
                                                                uint8_t* __restrict__ dst) {
    const int64_t total = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const int y0 = y * s, x0 = x * s, y1 = min(y0 + s, H), x1 = min(x0 + s, W);
        const unsigned first = src[(int64_t)y0 * W + x0];
        bool unlabelled = false, agree = true;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) {
                const unsigned v = src[(int64_t)yy * W + xx];
                unlabelled = unlabelled || v > 2u;
                agree = agree && v == first;
            }
        dst[i] = unlabelled ? (uint8_t)255 : (agree ? (uint8_t)first : (uint8_t)1);
    }
}

// ------------------------------------------------------------------------------------------------ coefficients
__device__ __forceinline__ unsigned quant16(float v) {
    return (unsigned)(int)(fminf(fmaxf(v, 0.f), 1.f) * 65535.f + 0.5f);
}

template <int C>
__global__ __launch_bounds__(256) void guided_raw_kernel(const otvm_guided_params p, float* __restrict__ raw) {
    __shared__ unsigned sI[TILE_MAX];
    __shared__ unsigned short sP[C][TILE_MAX];
    const int r = p.r, h = p.h, w = p.w;
    const int tw = TX + 2 * r, th = TY + 2 * r;
    const int bx0 = (int)blockIdx.x * TX - r, by0 = (int)blockIdx.y * TY - r;
    for (int i = threadIdx.x; i < tw * th; i += 256) {
        const int ly = i / tw, lx = i - ly * tw, gy = by0 + ly, gx = bx0 + lx;
        unsigned v = 0;
        unsigned q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const int64_t j = (int64_t)gy * w + gx;
            const uint8_t* g = p.guide_work + j * 3;
            v = (unsigned)g[0] | ((unsigned)g[1] << 8) | ((unsigned)g[2] << 16);
#pragma unroll
            for (int c = 0; c < C; ++c) q[c] = quant16(p.target[c][j]);
        }
        sI[i] = v;
#pragma unroll
        for (int c = 0; c < C; ++c) sP[c][i] = (unsigned short)q[c];
    }
    __syncthreads();
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int x = (int)blockIdx.x * TX + tx, y = (int)blockIdx.y * TY + ty;
    if (x >= w || y >= h) return;
    // the clipped window in tile coordinates (pixel (x, y) sits at (tx + r, ty + r))
    const int xa = max(x - r, 0), xb = min(x + r, w - 1), ya = max(y - r, 0), yb = min(y + r, h - 1);
    const int N = (xb - xa + 1) * (yb - ya + 1);
    unsigned S0 = 0, S1 = 0, S2 = 0, S00 = 0, S01 = 0, S02 = 0, S11 = 0, S12 = 0, S22 = 0;
    unsigned SP[C], SIP[C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) SP[c] = SIP[c][0] = SIP[c][1] = SIP[c][2] = 0;
    for (int gy = ya; gy <= yb; ++gy) {
        const int base = (gy - by0) * tw - bx0;
        for (int gx = xa; gx <= xb; ++gx) {
            const unsigned v = sI[base + gx];
            const unsigned i0 = v & 255u, i1 = (v >> 8) & 255u, i2 = v >> 16;
            S0 += i0; S1 += i1; S2 += i2;
            S00 += i0 * i0; S01 += i0 * i1; S02 += i0 * i2; S11 += i1 * i1; S12 += i1 * i2; S22 += i2 * i2;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const unsigned q = sP[c][base + gx];
                SP[c] += q;
                SIP[c][0] += i0 * q; SIP[c][1] += i1 * q; SIP[c][2] += i2 * q;
            }
        }
    }
    // fp64 from the exact integer numerators N * sum(I_c I_d) - sum(I_c) sum(I_d), scaled to the [0,1] range
    const int64_t n = N;
    const double dI = (double)(n * n * 65025), dP = (double)(n * n * 255 * 65535), dn = (double)N;
    const double s00 = (double)(n * S00 - (int64_t)S0 * S0) / dI + p.eps;
    const double s01 = (double)(n * S01 - (int64_t)S0 * S1) / dI;
    const double s02 = (double)(n * S02 - (int64_t)S0 * S2) / dI;
    const double s11 = (double)(n * S11 - (int64_t)S1 * S1) / dI + p.eps;
    const double s12 = (double)(n * S12 - (int64_t)S1 * S2) / dI;
    const double s22 = (double)(n * S22 - (int64_t)S2 * S2) / dI + p.eps;
    const double c00 = s11 * s22 - s12 * s12;
    const double c01 = s02 * s12 - s01 * s22;
    const double c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02;
    const double c12 = s01 * s02 - s00 * s12;
    const double c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    const double m0 = ((double)S0 / dn) / 255.0, m1 = ((double)S1 / dn) / 255.0, m2 = ((double)S2 / dn) / 255.0;
    f32x4* out = reinterpret_cast<f32x4*>(raw) + ((int64_t)y * w + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double p0 = (double)(n * SIP[c][0] - (int64_t)S0 * SP[c]) / dP;
        const double p1 = (double)(n * SIP[c][1] - (int64_t)S1 * SP[c]) / dP;
        const double p2 = (double)(n * SIP[c][2] - (int64_t)S2 * SP[c]) / dP;
        const double a0 = ((c00 * p0 + c01 * p1) + c02 * p2) / det;
        const double a1 = ((c01 * p0 + c11 * p1) + c12 * p2) / det;
        const double a2 = ((c02 * p0 + c12 * p1) + c22 * p2) / det;
        const double mP = ((double)SP[c] / dn) / 65535.0;
        const double b = mP - ((a0 * m0 + a1 * m1) + a2 * m2);
        out[c] = f32x4{(float)a0, (float)a1, (float)a2, (float)b};
    }
}

// box mean of target blockIdx.z's four coefficients over the same clipped window
__global__ __launch_bounds__(256) void guided_mean_kernel(const float* __restrict__ raw, int h, int w, int r, int C,
                                                          float* __restrict__ mean) {
    __shared__ double sR[(TY + 2 * RMAX) * TX][4];
    const int c = blockIdx.z;
    const int bx = (int)blockIdx.x * TX, by0 = (int)blockIdx.y * TY - r, th = TY + 2 * r;
    const f32x4* src = reinterpret_cast<const f32x4*>(raw);
    for (int i = threadIdx.x; i < th * TX; i += 256) {
        const int ly = i / TX, lx = i - ly * TX, gy = by0 + ly, gx = bx + lx;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (gy >= 0 && gy < h && gx < w) {
            const int xa = max(gx - r, 0), xb = min(gx + r, w - 1);
            for (int xx = xa; xx <= xb; ++xx) {
                const f32x4 v = src[((int64_t)gy * w + xx) * C + c];
                a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
            }
        }
        sR[i][0] = a0; sR[i][1] = a1; sR[i][2] = a2; sR[i][3] = a3;
    }
    __syncthreads();
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int x = bx + tx, y = (int)blockIdx.y * TY + ty;
    if (x >= w || y >= h) return;
    const int xa = max(x - r, 0), xb = min(x + r, w - 1), ya = max(y - r, 0), yb = min(y + r, h - 1);
    const double dn = (double)((xb - xa + 1) * (yb - ya + 1));
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int gy = ya; gy <= yb; ++gy) {
        const double* row = sR[(gy - by0) * TX + tx];
        a0 += row[0]; a1 += row[1]; a2 += row[2]; a3 += row[3];
    }
    reinterpret_cast<f32x4*>(mean)[((int64_t)y * w + x) * C + c] =
        f32x4{(float)(a0 / dn), (float)(a1 / dn), (float)(a2 / dn), (float)(a3 / dn)};
}

// ------------------------------------------------------------------------------------------------ apply
// half-pixel centres in integers: t = 2 X + 1 - s, x0 = floor(t / 2s), fx = (t - 2s x0) / 2s; t >= 1 - s > -2s
__device__ __forceinline__ void sample_of(int X, int s, int lim, int& ia, int& ib, float& f) {
    const int t = 2 * X + 1 - s, d = 2 * s;
    const int q = t >= 0 ? t / d : -1;
    f = (float)(t - d * q) / (float)d;
    ia = min(max(q, 0), lim - 1);
    ib = min(max(q + 1, 0), lim - 1);
}

__device__ __forceinline__ float lerp1(float u, float v, float f) { return u + f * (v - u); }

template <int C>
__global__ __launch_bounds__(256) void guided_apply_kernel(const otvm_guided_params p, const int vec) {
    const int H = p.H, W = p.W, s = p.s, h = p.h, w = p.w;
    const int n4 = (W + 3) >> 2;
    const int64_t total = (int64_t)H * n4, NP = (int64_t)H * W;
    const float k255 = 1.f / 255.f;
    const f32x4* coef = reinterpret_cast<const f32x4*>(p.coef);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = W - x0 < 4 ? W - x0 : 4;
        const int64_t o = (int64_t)y * W + x0;
        const bool full = n == 4 && vec;
        unsigned by[12];
        if (full) {
            const unsigned* g = reinterpret_cast<const unsigned*>(p.guide_full + o * 3);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const unsigned v = g[d];
#pragma unroll
                for (int j = 0; j < 4; ++j) by[4 * d + j] = (v >> (8 * j)) & 255u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) by[j] = j < 3 * n ? (unsigned)p.guide_full[o * 3 + j] : 0u;
        }
        int ya, yb;
        float fy;
        sample_of(y, s, h, ya, yb, fy);
        int64_t j00[4], j01[4], j10[4], j11[4];
        float fx[4], I0[4], I1[4], I2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int xa, xb;
            sample_of(min(x0 + k, W - 1), s, w, xa, xb, fx[k]);
            I0[k] = (float)by[3 * k] * k255; I1[k] = (float)by[3 * k + 1] * k255; I2[k] = (float)by[3 * k + 2] * k255;
            j00[k] = ((int64_t)ya * w + xa) * C; j01[k] = ((int64_t)ya * w + xb) * C;
            j10[k] = ((int64_t)yb * w + xa) * C; j11[k] = ((int64_t)yb * w + xb) * C;
        }
        // one target at a time (a rolled loop: the sixteen coefficient quads of ONE target are in flight, not of all four)
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            float res[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 c00 = coef[j00[k] + c], c01 = coef[j01[k] + c], c10 = coef[j10[k] + c], c11 = coef[j11[k] + c];
                float v[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float top = lerp1(c00[m], c01[m], fx[k]), bot = lerp1(c10[m], c11[m], fx[k]);
                    v[m] = lerp1(top, bot, fy);
                }
                const float q = ((v[0] * I0[k] + v[1] * I1[k]) + v[2] * I2[k]) + v[3];
                // NaN (non-finite coefficients: an eps too small for a constant guide region) -> 0 by an explicit select
                res[k] = !(q == q) ? 0.f : (q < 0.f ? 0.f : (q > 1.f ? 1.f : q));
            }
            float* dst = c == 0 ? p.alpha + o : p.fgr + (int64_t)(c - 1) * NP + o;
            if (full) {
                *reinterpret_cast<f32x4*>(dst) = f32x4{res[0], res[1], res[2], res[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) dst[k] = res[k];
            }
            if (c == 0 && p.alpha_u8) {
                unsigned a8[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) a8[k] = (unsigned)(uint8_t)(res[k] * 255.f);       // truncation, as otvm_crop_outputs
                if (full) {
                    *reinterpret_cast<unsigned*>(p.alpha_u8 + o) = a8[0] | (a8[1] << 8) | (a8[2] << 16) | (a8[3] << 24);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) p.alpha_u8[o + k] = (uint8_t)a8[k];
                }
            }
        }
    }
}

int check_sizes(const char* who, int H, int W, int s, int h, int w) {
    OTVM_REQUIRE(s >= 2 && s <= 4, "%s: the scale must be 2, 3 or 4, got %d", who, s);
    OTVM_REQUIRE(H > 0 && W > 0 && h == (H + s - 1) / s && w == (W + s - 1) / s,
                 "%s: the working size of %dx%d at scale %d is %dx%d, got %dx%d", who, W, H, s, (W + s - 1) / s, (H + s - 1) / s, w, h);
    return 0;
}

}  // namespace

extern "C" int otvm_downsample_u8(const uint8_t* src, int H, int W, int s, uint8_t* dst, void* stream) {
    OTVM_REQUIRE(src && dst && H > 0 && W > 0 && s >= 2 && s <= 4, "otvm_downsample_u8: null pointer, empty image or scale outside 2..4");
    const int h = (H + s - 1) / s, w = (W + s - 1) / s;
    hipLaunchKernelGGL(downsample_u8_kernel, dim3(grid_1d((int64_t)h * w)), dim3(256), 0, (hipStream_t)stream, src, H, W, s, h, w, dst);
    OTVM_CHECK_LAUNCH("otvm_downsample_u8");
    return 0;
}

extern "C" int otvm_downsample_trimap(const float* src, int H, int W, int s, float* dst, void* stream) {
    OTVM_REQUIRE(src && dst && H > 0 && W > 0 && s >= 2 && s <= 4,
                 "otvm_downsample_trimap: null pointer, empty image or scale outside 2..4");
    const int h = (H + s - 1) / s, w = (W + s - 1) / s;
    hipLaunchKernelGGL(downsample_trimap_kernel, dim3(grid_1d((int64_t)h * w)), dim3(256), 0, (hipStream_t)stream, src, H, W, s, h, w,
                       dst);
    OTVM_CHECK_LAUNCH("otvm_downsample_trimap");
    return 0;
}

extern "C" int otvm_downsample_labels(const uint8_t* src, int H, int W, int s, uint8_t* dst, void* stream) {
    OTVM_REQUIRE(src && dst && H > 0 && W > 0 && s >= 2 && s <= 4,
                 "otvm_downsample_labels: null pointer, empty image or scale outside 2..4");
    const int h = (H + s - 1) / s, w = (W + s - 1) / s;
    hipLaunchKernelGGL(downsample_labels_kernel, dim3(grid_1d((int64_t)h * w)), dim3(256), 0, (hipStream_t)stream, src, H, W, s, h, w,
                       dst);
    OTVM_CHECK_LAUNCH("otvm_downsample_labels");
    return 0;
}

extern "C" int64_t otvm_guided_ws_bytes(int h, int w, int C) {
    if (h < 1 || w < 1 || (C != 1 && C != 4)) return -1;
    return (int64_t)h * w * C * 16;
}

extern "C" int otvm_guided_coeffs(const otvm_guided_params* p, void* ws, void* stream) {
    OTVM_REQUIRE(p && ws && p->guide_work && p->coef, "otvm_guided_coeffs: null parameters / guide_work / coef / workspace");
    if (int rc = check_sizes("otvm_guided_coeffs", p->H, p->W, p->s, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->r >= 1 && p->r <= RMAX, "otvm_guided_coeffs: the radius must be 1..%d, got %d", RMAX, p->r);
    OTVM_REQUIRE(p->C == 1 || p->C == 4, "otvm_guided_coeffs: 1 target (alpha) or 4 (alpha + F), got %d", p->C);
    OTVM_REQUIRE(p->eps > 0.0 && p->eps < __builtin_inf(), "otvm_guided_coeffs: eps must be positive and finite");
    for (int c = 0; c < p->C; ++c) OTVM_REQUIRE(p->target[c], "otvm_guided_coeffs: target plane %d is null", c);
    OTVM_REQUIRE((((uintptr_t)ws | (uintptr_t)p->coef) & 15) == 0, "otvm_guided_coeffs: ws / coef must be 16-byte aligned");
    const dim3 grid((unsigned)otvm_ceil_div(p->w, TX), (unsigned)otvm_ceil_div(p->h, TY), 1);
    OTVM_REQUIRE(grid.y <= 65535u, "otvm_guided_coeffs: working height %d is too large", p->h);
    if (p->C == 1)
        hipLaunchKernelGGL(guided_raw_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, *p, (float*)ws);
    else
        hipLaunchKernelGGL(guided_raw_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, *p, (float*)ws);
    hipLaunchKernelGGL(guided_mean_kernel, dim3(grid.x, grid.y, (unsigned)p->C), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                       p->h, p->w, p->r, p->C, p->coef);
    OTVM_CHECK_LAUNCH("otvm_guided_coeffs");
    return 0;
}

extern "C" int otvm_guided_apply(const otvm_guided_params* p, void* stream) {
    OTVM_REQUIRE(p && p->guide_full && p->coef && p->alpha, "otvm_guided_apply: null parameters / guide_full / coef / alpha");
    if (int rc = check_sizes("otvm_guided_apply", p->H, p->W, p->s, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->C == 1 || p->C == 4, "otvm_guided_apply: 1 target (alpha) or 4 (alpha + F), got %d", p->C);
    OTVM_REQUIRE(p->C == 1 || p->fgr, "otvm_guided_apply: 4 targets need the fgr output planes");
    OTVM_REQUIRE(((uintptr_t)p->coef & 15) == 0 && (((uintptr_t)p->alpha | (uintptr_t)p->fgr) & 3) == 0,
                 "otvm_guided_apply: coef must be 16-byte, alpha / fgr 4-byte aligned");
    const int vec = (p->W & 3) == 0 && (((uintptr_t)p->alpha | (uintptr_t)p->fgr) & 15) == 0 &&
                    (((uintptr_t)p->alpha_u8 | (uintptr_t)p->guide_full) & 3) == 0;
    const unsigned grid = grid_1d((int64_t)p->H * ((p->W + 3) / 4));
    if (p->C == 1)
        hipLaunchKernelGGL(guided_apply_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *p, vec);
    else
        hipLaunchKernelGGL(guided_apply_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *p, vec);
    OTVM_CHECK_LAUNCH("otvm_guided_apply");
    return 0;
}
