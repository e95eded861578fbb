// Farneback dense optical flow on device -- OpenCV 4.x calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 10, 2, 7, 1.5,
// OPTFLOW_FARNEBACK_GAUSSIAN), the arguments of the reference's calcOpticalFlow (utils/tmp/metric.py:48-53) -- and the MESSDdt
// matting metric built on it (metric.py:266-302).  Compiled with -ffp-contract=off: every float32 operation below is one
// IEEE operation in the order tests/farneback_ref.py states.
//
// Per pyramid level k = L .. 0 (scale 0.5^k; L = the first k at which a side drops below 32, at most 5), for both frames:
//   rowblur   : the row pass of GaussianBlur(ksize, sigma, REFLECT_101) of the full-resolution frame, only at the source
//               columns the INTER_LINEAR resize to the level reads (two per output column; every column at level 0)
//   colblur   : the column pass at the two source rows of each output row, then the resize (OpenCV's area path for an exact
//               2x downscale).  At the coarse levels (ksize 39, 79) the blur is never evaluated on the whole frame.
//   polyexp   : FarnebackPolyExp(7, 1.5) on an LDS tile: vertical float32 pass, horizontal pass accumulated in double
// then, with the previous level's flow resized and doubled as the initial flow (zero at level L):
//   update    : FarnebackUpdateMatrices -> M (five planes)
//   blursolve : 11-tap Gaussian of M (vertical, then horizontal, replicated border) on an LDS tile and the 2x2 solve in double
//   update    : again from the new flow, between the two iterations
// OpenCV interleaves the second matrix update with the blur in stripes that lag 10 rows behind; the blur reads 5 rows ahead,
// so every flow row is computed from the previous iteration's M: the sweep IS a full blur + solve followed by a full update.
// No atomics: two calls give equal bits.
#include "common.h"
#include <math.h>

namespace {

constexpr int FB_MAX_LEVELS = 6;     // k = 0 .. 5
constexpr int FB_MAXK = 79;          // largest GaussianBlur ksize (level 5)
constexpr int FB_N = 7;              // poly_n
constexpr int FB_M = 5;              // winsize / 2
constexpr int FB_TX = 32, FB_TY = 16;  // output tile of the LDS kernels (block 32 x 8, two rows per thread)

struct FbLevel { int k, w, h, ksize; double sigma; };
struct FbTable { int n; FbLevel lv[FB_MAX_LEVELS]; };        // processing order: k = L first
struct FbBlurTaps { float k[FB_MAXK]; };
struct FbPolyTaps { float g[FB_N + 1], xg[FB_N + 1], xxg[FB_N + 1]; double ig11, ig03, ig33, ig55; };
struct FbWinTaps { float k[FB_M + 1]; };

// ---- host side constants (exported for the tests: otvm_optflow_farneback_params)
inline int fb_round(double x) { return (int)nearbyint(x); }   // cvRound: half to even

FbTable fb_table(int H, int W) {
    double scale = 1;
    int k = 0;
    for (; k < 5; ++k) {
        scale *= 0.5;
        if (W * scale < 32 || H * scale < 32) break;
    }
    FbTable t;
    t.n = k + 1;
    for (int i = 0; i <= k; ++i) {
        const int lv = k - i;
        double s = 1;
        for (int j = 0; j < lv; ++j) s *= 0.5;
        const double sigma = (1. / s - 1) * 0.5;
        int ks = fb_round(sigma * 5) | 1;
        ks = ks < 3 ? 3 : ks;
        t.lv[i] = FbLevel{lv, fb_round(W * s), fb_round(H * s), ks, sigma};
    }
    return t;
}

// getGaussianKernel: the fixed table for ksize 3 and sigma 0, else exp(-x^2 / (2 sigma^2)) normalised in double in OpenCV's
// bit-exact order (the half below the centre, doubled, plus the centre), stored as float32
void fb_gauss(int ks, double sigma, float* out) {
    if (sigma <= 0) { out[0] = 0.25f; out[1] = 0.5f; out[2] = 0.25f; return; }
    const int n2 = (ks - 1) / 2;
    const double scale2x = -0.125 / (sigma * sigma);
    double v[FB_MAXK / 2 + 1], s = 0;
    for (int i = 0; i < n2; ++i) {
        const int x = 1 - ks + 2 * i;
        v[i] = exp((double)(x * x) * scale2x);
        s += v[i];
    }
    s = s * 2.0 + 1.0;
    v[n2] = 1.0;
    for (int i = 0; i <= n2; ++i) out[i] = out[ks - 1 - i] = (float)(v[i] / s);
}

// FarnebackPrepareGaussian(7, 1.5): g, xg, xxg in float32; the moment matrix accumulated in double from float32 products; its
// inverse splits into 1/G11, 1/G55 and the 3x3 block on (0, 3, 4) = [[a, b, b], [b, c, d], [b, d, c]] solved in closed form
void fb_poly_taps(FbPolyTaps* t) {
    const int n = FB_N;
    const double sigma = 1.5;
    float g[2 * FB_N + 1];
    double s = 0;
    for (int x = -n; x <= n; ++x) {
        g[x + n] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; ++x) g[x + n] = (float)(g[x + n] * s);
    double G00 = 0, G11 = 0, G33 = 0, G55 = 0;
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const float gg = g[y + n] * g[x + n], fx = (float)x, fy = (float)y;
            G00 += gg;
            G11 += gg * fx * fx;
            G33 += gg * fx * fx * fx * fx;
            G55 += gg * fx * fx * fy * fy;
        }
    const double a = G00, b = G11, c = G33, d = G55;                 // G03 = G11, G34 = G55
    const double det = a * (c + d) - 2 * b * b;
    t->ig11 = 1.0 / G11;
    t->ig03 = -b / det;
    t->ig33 = 0.5 * (a / det + 1.0 / (c - d));
    t->ig55 = 1.0 / G55;
    for (int k = 0; k <= n; ++k) {
        t->g[k] = g[k + n];
        t->xg[k] = (float)k * g[k + n];
        t->xxg[k] = (float)(k * k) * g[k + n];
    }
}

// FarnebackUpdateFlow_GaussianBlur's 11-tap kernel (sigma = 5 * 0.3), centre first
void fb_win_taps(FbWinTaps* t) {
    const double sigma = FB_M * 0.3;
    double s = 1;
    float k[FB_M + 1];
    k[0] = 1.f;
    for (int i = 1; i <= FB_M; ++i) {
        k[i] = (float)exp(-i * i / (2 * sigma * sigma));
        s += k[i] * 2;
    }
    s = 1. / s;
    for (int i = 0; i <= FB_M; ++i) t->k[i] = (float)(k[i] * s);
}

// ---- device
__device__ __forceinline__ int fb_r101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * n - 2 - i;
    }
    return i;
}

// INTER_LINEAR source index pair and weights of output d along an axis of n_src (OpenCV's clamping: below 0 -> (0, fx 0),
// at or past the last pixel -> (last, fx 0))
__device__ __forceinline__ void fb_coeff(int d, double scale, int n_src, int& s0, int& s1, float& w0, float& w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    f = f - fl;
    int s = (int)fl;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
    s0 = s;
    s1 = s + 1 < n_src ? s + 1 : n_src - 1;
    w0 = 1.f - f;
    w1 = f;
}

// row pass of the Gaussian at the columns the resize reads: hb[z][y][j], j = 2 dx + e (two) or the column itself (level 0)
__global__ __launch_bounds__(256) void fb_rowblur_kernel(const uint8_t* __restrict__ img0, const uint8_t* __restrict__ img1, int H,
                                                         int W, int nc, int two, double scale_x, FbBlurTaps taps, int ks,
                                                         float* __restrict__ hb) {
    const int j = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (j >= nc) return;
    int c = j;
    if (two) {
        int s0, s1;
        float w0, w1;
        fb_coeff(j >> 1, scale_x, W, s0, s1, w0, w1);
        c = (j & 1) ? s1 : s0;
    }
    const uint8_t* src = (z ? img1 : img0) + (int64_t)y * W;
    float s;
    if (ks == 3) {
        s = (float)src[c] * taps.k[1] + ((float)src[fb_r101(c - 1, W)] + (float)src[fb_r101(c + 1, W)]) * taps.k[0];
    } else {
        const int r = ks >> 1;
        s = taps.k[0] * (float)src[fb_r101(c - r, W)];
        for (int q = 1; q < ks; ++q) s = s + taps.k[q] * (float)src[fb_r101(c - r + q, W)];
    }
    hb[((int64_t)z * H + y) * nc + j] = s;
}

__device__ __forceinline__ float fb_colf(const float* __restrict__ hb, int H, int nc, int row, int j, const FbBlurTaps& taps, int ks) {
    if (ks == 3)
        return (hb[(int64_t)fb_r101(row - 1, H) * nc + j] + hb[(int64_t)fb_r101(row + 1, H) * nc + j]) * taps.k[0] +
               hb[(int64_t)row * nc + j] * taps.k[1];
    const int r = ks >> 1;
    float s = taps.k[r] * hb[(int64_t)row * nc + j];
    for (int i = 1; i <= r; ++i)
        s = s + taps.k[r + i] * (hb[(int64_t)fb_r101(row + i, H) * nc + j] + hb[(int64_t)fb_r101(row - i, H) * nc + j]);
    return s;
}

// column pass at the rows the resize reads, then the resize: I[z][dy][dx] (w x h)
__global__ __launch_bounds__(256) void fb_colblur_kernel(const float* __restrict__ hb, int H, int W, int nc, int two, int area,
                                                         double scale_x, double scale_y, int w, int h, FbBlurTaps taps, int ks,
                                                         float* __restrict__ img) {
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    if (dx >= w || dy >= h) return;
    const float* b = hb + (int64_t)z * H * nc;
    float out;
    if (!two) {
        out = fb_colf(b, H, nc, dy, dx, taps, ks);
    } else {
        int sy0, sy1, sx0, sx1;
        float b0, b1, a0, a1;
        fb_coeff(dy, scale_y, H, sy0, sy1, b0, b1);
        fb_coeff(dx, scale_x, W, sx0, sx1, a0, a1);
        const float pa = fb_colf(b, H, nc, sy0, 2 * dx, taps, ks), pb = fb_colf(b, H, nc, sy0, 2 * dx + 1, taps, ks);
        const float pc = fb_colf(b, H, nc, sy1, 2 * dx, taps, ks), pd = fb_colf(b, H, nc, sy1, 2 * dx + 1, taps, ks);
        if (area) {
            out = ((pa + pb) + (pc + pd)) * 0.25f;
        } else {
            const float h0 = pa * a0 + pb * a1, h1 = pc * a0 + pd * a1;
            out = h0 * b0 + h1 * b1;
        }
    }
    img[((int64_t)z * h + dy) * w + dx] = out;
}

// FarnebackPolyExp(7, 1.5) of I[z] -> R[z] = five planes (y, x, yy, xx, xy) of w x h.  Block (32, 8), 32 x 16 outputs; the
// replicated borders of both passes are clamped loads (a column's vertical pass depends on that column alone)
__global__ __launch_bounds__(256) void fb_polyexp_kernel(const float* __restrict__ img, int w, int h, FbPolyTaps taps,
                                                         float* __restrict__ R) {
    constexpr int LX = FB_TX + 2 * FB_N, LY = FB_TY + 2 * FB_N;
    __shared__ float sin_[LY][LX];
    __shared__ float sv[3][FB_TY][LX];
    const int z = blockIdx.z, x0 = blockIdx.x * FB_TX, y0 = blockIdx.y * FB_TY;
    const int tid = threadIdx.y * FB_TX + threadIdx.x;
    const float* src = img + (int64_t)z * h * w;
    for (int e = tid; e < LY * LX; e += 256) {
        const int ry = e / LX, rx = e % LX;
        const int y = min(max(y0 + ry - FB_N, 0), h - 1), x = min(max(x0 + rx - FB_N, 0), w - 1);
        sin_[ry][rx] = src[(int64_t)y * w + x];
    }
    __syncthreads();
    for (int e = tid; e < FB_TY * LX; e += 256) {
        const int ry = e / LX, cx = e % LX;
        float r0 = sin_[ry + FB_N][cx] * taps.g[0], r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int k = 1; k <= FB_N; ++k) {
            const float s0 = sin_[ry + FB_N - k][cx], s1 = sin_[ry + FB_N + k][cx];
            const float p = s0 + s1;
            r0 = r0 + taps.g[k] * p;
            r1 = r1 + taps.xg[k] * (s1 - s0);
            r2 = r2 + taps.xxg[k] * p;
        }
        sv[0][ry][cx] = r0;
        sv[1][ry][cx] = r1;
        sv[2][ry][cx] = r2;
    }
    __syncthreads();
    const int c = threadIdx.x, x = x0 + c;
    float* dst = R + (int64_t)z * 5 * h * w;
    const int64_t plane = (int64_t)h * w;
#pragma unroll
    for (int q = 0; q < FB_TY / 8; ++q) {
        const int r = threadIdx.y + 8 * q, y = y0 + r;
        if (x >= w || y >= h) continue;
        const int cc = c + FB_N;
        double b1 = sv[0][r][cc] * taps.g[0], b2 = 0, b3 = sv[1][r][cc] * taps.g[0], b4 = 0, b5 = sv[2][r][cc] * taps.g[0], b6 = 0;
#pragma unroll
        for (int k = 1; k <= FB_N; ++k) {
            const double tg = sv[0][r][cc + k] + sv[0][r][cc - k];
            b1 += tg * (double)taps.g[k];
            b4 += tg * (double)taps.xxg[k];
            b2 += (double)((sv[0][r][cc + k] - sv[0][r][cc - k]) * taps.xg[k]);
            b3 += (double)((sv[1][r][cc + k] + sv[1][r][cc - k]) * taps.g[k]);
            b6 += (double)((sv[1][r][cc + k] - sv[1][r][cc - k]) * taps.xg[k]);
            b5 += (double)((sv[2][r][cc + k] + sv[2][r][cc - k]) * taps.g[k]);
        }
        const int64_t o = (int64_t)y * w + x;
        dst[o] = (float)(b3 * taps.ig11);
        dst[plane + o] = (float)(b2 * taps.ig11);
        dst[2 * plane + o] = (float)(b1 * taps.ig03 + b5 * taps.ig33);
        dst[3 * plane + o] = (float)(b1 * taps.ig03 + b4 * taps.ig33);
        dst[4 * plane + o] = (float)(b6 * taps.ig55);
    }
}

__device__ __forceinline__ float fb_border(int i) { return i < 2 ? 0.14f : 0.4472f; }

// FarnebackUpdateMatrices.  The flow is read from `flow` ([h][w][2]) or, for a level's first update, resized from the previous
// level's flow `pflow` (pw x ph) and doubled (neither: zero, the coarsest level)
__global__ __launch_bounds__(256) void fb_update_kernel(const float* __restrict__ R0, const float* __restrict__ R1, int w, int h,
                                                        const float* __restrict__ flow, const float* __restrict__ pflow, int pw, int ph,
                                                        float* __restrict__ M) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int64_t plane = (int64_t)h * w, o = (int64_t)y * w + x;
    float dx = 0.f, dy = 0.f;
    if (flow) {
        dx = flow[2 * o];
        dy = flow[2 * o + 1];
    } else if (pflow) {
        int sx0, sx1, sy0, sy1;
        float a0, a1, b0, b1;
        fb_coeff(x, 1.0 / ((double)w / pw), pw, sx0, sx1, a0, a1);
        fb_coeff(y, 1.0 / ((double)h / ph), ph, sy0, sy1, b0, b1);
        const float* p0 = pflow + (int64_t)sy0 * pw * 2;
        const float* p1 = pflow + (int64_t)sy1 * pw * 2;
        float v[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float h0 = p0[2 * sx0 + c] * a0 + p0[2 * sx1 + c] * a1;
            const float h1 = p1[2 * sx0 + c] * a0 + p1[2 * sx1 + c] * a1;
            v[c] = (h0 * b0 + h1 * b1) * 2.f;
        }
        dx = v[0];
        dy = v[1];
    }
    float fx = (float)x + dx, fy = (float)y + dy;
    const float x1 = floorf(fx), y1 = floorf(fy);
    fx = fx - x1;
    fy = fy - y1;
    const float r00 = R0[o], r01 = R0[plane + o], r02 = R0[2 * plane + o], r03 = R0[3 * plane + o], r04 = R0[4 * plane + o];
    float r2, r3, r4, r5, r6;
    if (x1 >= 0.f && x1 < (float)(w - 1) && y1 >= 0.f && y1 < (float)(h - 1)) {
        const int xi = (int)x1, yi = (int)y1;
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        float r[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float* p = R1 + c * plane + (int64_t)yi * w + xi;
            r[c] = ((a00 * p[0] + a01 * p[1]) + a10 * p[w]) + a11 * p[w + 1];
        }
        r2 = r[0];
        r3 = r[1];
        r4 = (r02 + r[2]) * 0.5f;
        r5 = (r03 + r[3]) * 0.5f;
        r6 = (r04 + r[4]) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = r02;
        r5 = r03;
        r6 = r04 * 0.5f;
    }
    r2 = (r00 - r2) * 0.5f;
    r3 = (r01 - r3) * 0.5f;
    r2 = r2 + (r4 * dy + r6 * dx);
    r3 = r3 + (r6 * dy + r5 * dx);
    const float scale = (((x < 5 ? fb_border(x) : 1.f) * (x >= w - 5 ? fb_border(w - x - 1) : 1.f)) * (y < 5 ? fb_border(y) : 1.f)) *
                        (y >= h - 5 ? fb_border(h - y - 1) : 1.f);
    r2 = r2 * scale; r3 = r3 * scale; r4 = r4 * scale; r5 = r5 * scale; r6 = r6 * scale;
    M[o] = r4 * r4 + r6 * r6;
    M[plane + o] = (r4 + r5) * r6;
    M[2 * plane + o] = r5 * r5 + r6 * r6;
    M[3 * plane + o] = r4 * r2 + r6 * r3;
    M[4 * plane + o] = r6 * r2 + r5 * r3;
}

// blur of M (11 taps, vertical then horizontal, replicated border) and the solve in double -> flow [h][w][2]
__global__ __launch_bounds__(256) void fb_blursolve_kernel(const float* __restrict__ M, int w, int h, FbWinTaps taps,
                                                           float* __restrict__ flow) {
    constexpr int LX = FB_TX + 2 * FB_M, LY = FB_TY + 2 * FB_M;
    __shared__ float sm[5][LY][LX];
    __shared__ float sv[5][FB_TY][LX];
    const int x0 = blockIdx.x * FB_TX, y0 = blockIdx.y * FB_TY;
    const int tid = threadIdx.y * FB_TX + threadIdx.x;
    const int64_t plane = (int64_t)h * w;
    for (int e = tid; e < LY * LX; e += 256) {
        const int ry = e / LX, rx = e % LX;
        const int y = min(max(y0 + ry - FB_M, 0), h - 1), x = min(max(x0 + rx - FB_M, 0), w - 1);
        const int64_t o = (int64_t)y * w + x;
#pragma unroll
        for (int c = 0; c < 5; ++c) sm[c][ry][rx] = M[c * plane + o];
    }
    __syncthreads();
    for (int e = tid; e < FB_TY * LX; e += 256) {
        const int ry = e / LX, cx = e % LX;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            float s = sm[c][ry + FB_M][cx] * taps.k[0];
#pragma unroll
            for (int i = 1; i <= FB_M; ++i) s = s + (sm[c][ry + FB_M + i][cx] + sm[c][ry + FB_M - i][cx]) * taps.k[i];
            sv[c][ry][cx] = s;
        }
    }
    __syncthreads();
    const int cx = threadIdx.x, x = x0 + cx;
#pragma unroll
    for (int q = 0; q < FB_TY / 8; ++q) {
        const int r = threadIdx.y + 8 * q, y = y0 + r;
        if (x >= w || y >= h) continue;
        double g[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            float s = sv[c][r][cx + FB_M] * taps.k[0];
#pragma unroll
            for (int i = 1; i <= FB_M; ++i) s = s + taps.k[i] * (sv[c][r][cx + FB_M - i] + sv[c][r][cx + FB_M + i]);
            g[c] = s;
        }
        const double idet = 1. / (g[0] * g[2] - g[1] * g[1] + 1e-3);
        const int64_t o = (int64_t)y * w + x;
        flow[2 * o] = (float)((g[0] * g[4] - g[1] * g[3]) * idet);
        flow[2 * o + 1] = (float)((g[2] * g[3] - g[1] * g[4]) * idet);
    }
}

// MESSDdt terms of one pair with the reference's transposed lookup: pixel (r, c) of frame 1 is read at row
// clamp(c + rint(dx), 0, H-1), column clamp(r + rint(dy), 0, W-1).  |(p0-t0)^2 m0 - (p1w-t1w)^2 m1w| and m0 are integers:
// block partials of 32 x 32 tiles in fp64 are exact, summed in a fixed order by ms_finish_kernel
__device__ __forceinline__ int64_t ms_rint(float v) {
    double d = rint((double)v);
    if (!(d >= -1e9)) d = -1e9;                       // NaN: numpy's int64 cast gives INT64_MIN, clamped to 0 just the same
    if (d > 1e9) d = 1e9;
    return (int64_t)d;
}

__global__ __launch_bounds__(256) void ms_terms_kernel(const uint8_t* __restrict__ p0, const uint8_t* __restrict__ t0,
                                                       const uint8_t* __restrict__ m0, const uint8_t* __restrict__ p1,
                                                       const uint8_t* __restrict__ t1, const uint8_t* __restrict__ m1, int H, int W,
                                                       const float* __restrict__ flow, double* __restrict__ part) {
    __shared__ double red[2][256];
    const int tid = threadIdx.y * 32 + threadIdx.x, c = blockIdx.x * 32 + threadIdx.x;
    double se = 0, sm = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = blockIdx.y * 32 + threadIdx.y + 8 * q;
        if (c >= W || r >= H) continue;
        const int64_t o = (int64_t)r * W + c;
        int64_t row = (int64_t)c + ms_rint(flow[2 * o]), col = (int64_t)r + ms_rint(flow[2 * o + 1]);
        row = row < 0 ? 0 : (row > H - 1 ? H - 1 : row);
        col = col < 0 ? 0 : (col > W - 1 ? W - 1 : col);
        const int64_t g = row * W + col;
        const int ma = m0 ? (m0[o] != 0) : 1, mb = m1 ? (m1[g] != 0) : 1;
        const int d0 = (int)p0[o] - (int)t0[o], d1 = (int)p1[g] - (int)t1[g];
        const int e = d0 * d0 * ma - d1 * d1 * mb;
        se += (double)(e < 0 ? -e : e);
        sm += (double)ma;
    }
    red[0][tid] = se;
    red[1][tid] = sm;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * b] = red[0][0];
        part[2 * b + 1] = red[1][0];
    }
}

__global__ __launch_bounds__(256) void ms_finish_kernel(const double* __restrict__ part, int nb, double* __restrict__ acc) {
    __shared__ double red[2][256];
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += part[2 * i]; b += part[2 * i + 1]; }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { acc[0] += red[0][0]; acc[1] += red[1][0]; }
}

inline int64_t fb_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct FbWs { float *hb, *img, *R, *M, *flow[2], *own; double* part; int64_t bytes; };

// every buffer sized for level 0 (the largest): hb holds H rows of at most W + 1 columns per frame
FbWs fb_ws_layout(int H, int W, void* base) {
    const int64_t N = (int64_t)H * W, nb = (int64_t)otvm_ceil_div(W, 32) * otvm_ceil_div(H, 32);
    const uintptr_t b = (uintptr_t)base;
    FbWs w;
    int64_t o = 0;
    w.hb = (float*)(b + o); o += fb_align(4 * 2 * (int64_t)H * (W + 2));
    w.img = (float*)(b + o); o += fb_align(4 * 2 * N);
    w.R = (float*)(b + o); o += fb_align(4 * 10 * N);
    w.M = (float*)(b + o); o += fb_align(4 * 5 * N);
    w.flow[0] = (float*)(b + o); o += fb_align(4 * 2 * N);
    w.flow[1] = (float*)(b + o); o += fb_align(4 * 2 * N);
    w.own = (float*)(b + o); o += fb_align(4 * 2 * N);
    w.part = (double*)(b + o); o += fb_align(16 * nb);
    w.bytes = o;
    return w;
}

int fb_run(const uint8_t* prev, const uint8_t* next, int H, int W, float* flow_out, const FbWs& ws, hipStream_t s) {
    static FbPolyTaps poly;
    static FbWinTaps win;
    static const bool init = (fb_poly_taps(&poly), fb_win_taps(&win), true);
    (void)init;
    const FbTable t = fb_table(H, W);
    const float* pflow = nullptr;
    int pw = 0, ph = 0;
    for (int i = 0; i < t.n; ++i) {
        const FbLevel& L = t.lv[i];
        FbBlurTaps taps;
        fb_gauss(L.ksize, L.k == 0 ? 0.0 : L.sigma, taps.k);
        const int two = !(L.w == W && L.h == H);
        const int nc = two ? 2 * L.w : W;
        const int area = two && W == 2 * L.w && H == 2 * L.h;
        const double sx = 1.0 / ((double)L.w / W), sy = 1.0 / ((double)L.h / H);
        hipLaunchKernelGGL(fb_rowblur_kernel, dim3(otvm_ceil_div(nc, 256), H, 2), dim3(256), 0, s, prev, next, H, W, nc, two, sx, taps,
                           L.ksize, ws.hb);
        const dim3 pix(otvm_ceil_div(L.w, 64), otvm_ceil_div(L.h, 4));
        hipLaunchKernelGGL(fb_colblur_kernel, dim3(pix.x, pix.y, 2), dim3(256), 0, s, (const float*)ws.hb, H, W, nc, two, area, sx, sy,
                           L.w, L.h, taps, L.ksize, ws.img);
        const dim3 tiles(otvm_ceil_div(L.w, FB_TX), otvm_ceil_div(L.h, FB_TY));
        hipLaunchKernelGGL(fb_polyexp_kernel, dim3(tiles.x, tiles.y, 2), dim3(FB_TX, 8), 0, s, (const float*)ws.img, L.w, L.h, poly, ws.R);
        const float* R0 = ws.R;
        const float* R1 = ws.R + (int64_t)5 * L.w * L.h;
        float* cur = L.k == 0 ? flow_out : ws.flow[i & 1];
        hipLaunchKernelGGL(fb_update_kernel, pix, dim3(256), 0, s, R0, R1, L.w, L.h, (const float*)nullptr, pflow, pw, ph, ws.M);
        for (int it = 0; it < 2; ++it) {
            hipLaunchKernelGGL(fb_blursolve_kernel, tiles, dim3(FB_TX, 8), 0, s, (const float*)ws.M, L.w, L.h, win, cur);
            if (it == 0)
                hipLaunchKernelGGL(fb_update_kernel, pix, dim3(256), 0, s, R0, R1, L.w, L.h, (const float*)cur, (const float*)nullptr, 0, 0,
                                   ws.M);
        }
        OTVM_CHECK_LAUNCH("otvm_optflow_farneback");
        pflow = cur;
        pw = L.w;
        ph = L.h;
    }
    return 0;
}

}  // namespace

extern "C" int otvm_optflow_farneback_params(int H, int W, int* levels, float* blur_taps, float* poly_taps, double* poly_inv,
                                             float* win_taps) {
    if (H <= 0 || W <= 0) return -1;
    const FbTable t = fb_table(H, W);
    for (int i = 0; i < t.n; ++i) {
        const FbLevel& L = t.lv[i];
        if (levels) { levels[4 * i] = L.k; levels[4 * i + 1] = L.w; levels[4 * i + 2] = L.h; levels[4 * i + 3] = L.ksize; }
        if (blur_taps) {
            for (int q = 0; q < FB_MAXK; ++q) blur_taps[FB_MAXK * i + q] = 0.f;
            fb_gauss(L.ksize, L.k == 0 ? 0.0 : L.sigma, blur_taps + FB_MAXK * i);
        }
    }
    FbPolyTaps p;
    fb_poly_taps(&p);
    if (poly_taps)
        for (int k = 0; k <= FB_N; ++k) { poly_taps[k] = p.g[k]; poly_taps[FB_N + 1 + k] = p.xg[k]; poly_taps[2 * (FB_N + 1) + k] = p.xxg[k]; }
    if (poly_inv) { poly_inv[0] = p.ig11; poly_inv[1] = p.ig03; poly_inv[2] = p.ig33; poly_inv[3] = p.ig55; }
    if (win_taps) {
        FbWinTaps wt;
        fb_win_taps(&wt);
        for (int i = 0; i <= FB_M; ++i) win_taps[i] = wt.k[i];
    }
    return t.n;
}

extern "C" int64_t otvm_optflow_farneback_ws_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return fb_ws_layout(H, W, nullptr).bytes;
}

extern "C" int otvm_optflow_farneback(const uint8_t* prev, const uint8_t* next, int H, int W, float* flow, void* ws, void* stream) {
    OTVM_REQUIRE(prev && next && flow && ws && H > 0 && W > 0, "otvm_optflow_farneback: bad arguments");
    OTVM_REQUIRE(H <= 65535, "otvm_optflow_farneback: H = %d exceeds the grid's row limit", H);
    return fb_run(prev, next, H, W, flow, fb_ws_layout(H, W, ws), (hipStream_t)stream);
}

extern "C" int otvm_matting_messddt(const uint8_t* p0, const uint8_t* t0, const uint8_t* m0, const uint8_t* p1, const uint8_t* t1,
                                    const uint8_t* m1, int H, int W, double* acc, float* flow_out, void* ws, void* stream) {
    OTVM_REQUIRE(p0 && t0 && p1 && t1 && acc && ws && H > 0 && W > 0, "otvm_matting_messddt: bad arguments");
    OTVM_REQUIRE(H <= 65535, "otvm_matting_messddt: H = %d exceeds the grid's row limit", H);
    hipStream_t s = (hipStream_t)stream;
    const FbWs w = fb_ws_layout(H, W, ws);
    float* flow = flow_out ? flow_out : w.own;
    const int rc = fb_run(t0, t1, H, W, flow, w, s);
    if (rc) return rc;
    const dim3 tiles(otvm_ceil_div(W, 32), otvm_ceil_div(H, 32));
    hipLaunchKernelGGL(ms_terms_kernel, tiles, dim3(32, 8), 0, s, p0, t0, m0, p1, t1, m1, H, W, (const float*)flow, w.part);
    hipLaunchKernelGGL(ms_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)w.part, (int)(tiles.x * tiles.y), acc);
    OTVM_CHECK_LAUNCH("otvm_matting_messddt");
    return 0;
}
