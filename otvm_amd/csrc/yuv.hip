// Video streams (include/otvm_hip.h: otvm_yuv_to_rgb, otvm_rgb_to_yuv420): 8-bit YUV as a decoder or a Y4M stream holds it <-> the
// uint8 [H,W,3] frames every other entry point takes.  Integer arithmetic only (the header states every operation and constant;
// tests/yuv_ref.py restates both kernels and is compared bit for bit), no atomics, no LDS.
//
// Both are streaming passes: at 1920x1080 a 4:2:0 frame is 3.1 MB, its RGB form 6.2 MB.  A thread owns a block of 4 x 2 luma
// samples, so that the chroma it needs -- at most 3 rows of 4 samples per plane for 4:2:0, clamped at the plane's edges -- is
// loaded once and serves eight pixels, and the two rows of a 2 x 2 chroma block are summed by the thread that loaded them.  Four
// pixels of a row are one dword of Y and three dwords of RGB: a row of the block moves as dwords when the block lies inside the
// image and the row's address is dword-aligned (decided per row from the address itself: any stride, any base, any W is taken),
// and byte by byte otherwise -- the ragged right and bottom edges included.  Row offsets are 64-bit.
#include "common.h"

namespace {

struct YuvInv { int cy, rv, gu, gv, bu; };          // YUV -> RGB, 20 fractional bits; the chroma ones act on 16 x chroma
struct YuvFwd { int yr, yg, yb, ch, ur, vb; };      // RGB -> YUV, 20 fractional bits; ug = ch - ur, vg = ch - vb

// [matrix][range]: derived from (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722), limited = 219 / 255 (Y) and 224 / 255 (C)
constexpr YuvInv kInv[2][2] = {{{1220945, 104597, 25675, 53279, 132201}, {1048576, 91881, 22553, 46802, 116130}},
                               {{1220945, 117489, 13975, 34925, 138438}, {1048576, 103206, 12276, 30679, 121609}}};
constexpr YuvFwd kFwd[2][2] = {{{269262, 528618, 102662, 460551, 155423, 74897}, {313524, 615514, 119538, 524288, 176932, 85262}},
                               {{191455, 644068, 65019, 460551, 105533, 42230}, {222927, 749942, 75707, 524288, 120138, 48074}}};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool dword_aligned(const void* q) { return ((uintptr_t)q & 3) == 0; }

// twelve bytes <-> three dwords
__device__ __forceinline__ void unpack12(const uint8_t* q, int (&b)[12]) {
    const unsigned* w = reinterpret_cast<const unsigned*>(q);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const unsigned v = w[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[4 * i + j] = (int)((v >> (8 * j)) & 255u);
    }
}
__device__ __forceinline__ void pack12(uint8_t* q, const int (&b)[12]) {
    unsigned* w = reinterpret_cast<unsigned*>(q);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        w[i] = (unsigned)b[4 * i] | ((unsigned)b[4 * i + 1] << 8) | ((unsigned)b[4 * i + 2] << 16) | ((unsigned)b[4 * i + 3] << 24);
}

// SUBX / SUBY: chroma has half the columns / rows; MONO: no chroma.  up / vp and cstep (bytes between two samples of a row: 2 for
// NV12) are set by the host, so that planar and interleaved chroma are one body.
template <bool SUBX, bool SUBY, bool MONO>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const otvm_yuv_to_rgb_params p, const YuvInv k, const int yo,
                                                         const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp,
                                                         const int ustride, const int vstride, const int cstep) {
    constexpr int NR = SUBY ? 3 : 2;                 // chroma rows a block of two luma rows reads
    const int H = p.H, W = p.W;
    const int n4 = (W + 3) >> 2, n2 = (H + 1) >> 1;
    const int cw = SUBX ? (W + 1) >> 1 : W, chh = SUBY ? (H + 1) >> 1 : H;
    const bool centre = p.siting == OTVM_YUV_SITING_CENTRE;
    const int64_t total = (int64_t)n4 * n2;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int by = (int)(t / n4), x0 = (int)(t - (int64_t)by * n4) * 4, y0 = by * 2;
        const int n = W - x0 < 4 ? W - x0 : 4;
        int du[2][4], dv[2][4];
        if constexpr (MONO) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) du[r][j] = dv[r][j] = 0;
        } else {
            int hu[NR][4], hv[NR][4];                // 4 x chroma: the horizontal half of the interpolation, per chroma row
            const int c0 = x0 >> 1;
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const int row = SUBY ? clampi(by - 1 + q, 0, chh - 1) : clampi(y0 + q, 0, chh - 1);
                const uint8_t* ur = up + (int64_t)row * ustride;
                const uint8_t* vr = vp + (int64_t)row * vstride;
                int cu[4], cv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int col = SUBX ? clampi(c0 - 1 + i, 0, cw - 1) : clampi(x0 + i, 0, cw - 1);
                    cu[i] = ur[(int64_t)col * cstep];
                    cv[i] = vr[(int64_t)col * cstep];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (SUBX) {
                        const int a = (j >> 1) + 1;                      // cu[a] is C[x >> 1]
                        const int b = (j & 1) ? a + 1 : a - 1;
                        if (centre) {
                            hu[q][j] = 3 * cu[a] + cu[b];
                            hv[q][j] = 3 * cv[a] + cv[b];
                        } else {
                            hu[q][j] = (j & 1) ? 2 * cu[a] + 2 * cu[a + 1] : 4 * cu[a];
                            hv[q][j] = (j & 1) ? 2 * cv[a] + 2 * cv[a + 1] : 4 * cv[a];
                        }
                    } else {
                        hu[q][j] = 4 * cu[j];
                        hv[q][j] = 4 * cv[j];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (SUBY) {                      // hu[1] is row[y >> 1]; the even luma row leans up, the odd one down
                        du[r][j] = 3 * hu[1][j] + hu[r == 0 ? 0 : 2][j] - 2048;
                        dv[r][j] = 3 * hv[1][j] + hv[r == 0 ? 0 : 2][j] - 2048;
                    } else {
                        du[r][j] = 4 * hu[r][j] - 2048;
                        dv[r][j] = 4 * hv[r][j] - 2048;
                    }
                }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + r;
            if (y >= H) break;
            const uint8_t* yr = p.y + (int64_t)y * p.y_stride + x0;
            int yy[4];
            if (n == 4 && dword_aligned(yr)) {
                const unsigned v = *reinterpret_cast<const unsigned*>(yr);
#pragma unroll
                for (int j = 0; j < 4; ++j) yy[j] = (int)((v >> (8 * j)) & 255u);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) yy[j] = yr[j < n ? j : n - 1];
            }
            int b[12];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int l = k.cy * (yy[j] - yo) + (1 << 19);
                const int R = clampi((l + k.rv * dv[r][j]) >> 20, 0, 255);
                const int G = clampi((l - k.gu * du[r][j] - k.gv * dv[r][j]) >> 20, 0, 255);
                const int B = clampi((l + k.bu * du[r][j]) >> 20, 0, 255);
                b[3 * j] = p.u8_rgb ? R : B;
                b[3 * j + 1] = G;
                b[3 * j + 2] = p.u8_rgb ? B : R;
            }
            uint8_t* o = p.rgb + ((int64_t)y * W + x0) * 3;
            if (n == 4 && dword_aligned(o)) {
                pack12(o, b);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < 3 * n) o[j] = (uint8_t)b[j];
            }
        }
    }
}

__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const otvm_rgb_to_yuv420_params p, const YuvFwd k, const int yo) {
    const int H = p.H, W = p.W;
    const int n4 = (W + 3) >> 2, n2 = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int64_t total = (int64_t)n4 * n2;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int by = (int)(t / n4), x0 = (int)(t - (int64_t)by * n4) * 4, y0 = by * 2;
        const int n = W - x0 < 4 ? W - x0 : 4;
        int sR[2] = {0, 0}, sG[2] = {0, 0}, sB[2] = {0, 0};       // the two 2 x 2 blocks' sums
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + r, row = y < H ? y : H - 1;         // the bottom edge of an odd H counts its last row twice
            const uint8_t* q = p.img + ((int64_t)row * W + x0) * 3;
            int b[12];
            if (n == 4 && dword_aligned(q)) {
                unpack12(q, b);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = j < n ? j : n - 1;             // likewise the right edge of an odd W
#pragma unroll
                    for (int c = 0; c < 3; ++c) b[3 * j + c] = q[3 * col + c];
                }
            }
            int yy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int R = p.u8_rgb ? b[3 * j] : b[3 * j + 2], G = b[3 * j + 1], B = p.u8_rgb ? b[3 * j + 2] : b[3 * j];
                yy[j] = ((k.yr * R + k.yg * G + k.yb * B + (1 << 19)) >> 20) + yo;
                sR[j >> 1] += R;
                sG[j >> 1] += G;
                sB[j >> 1] += B;
            }
            if (y < H) {
                uint8_t* o = p.y + (int64_t)y * p.y_stride + x0;
                if (n == 4 && dword_aligned(o)) {
                    *reinterpret_cast<unsigned*>(o) = (unsigned)yy[0] | ((unsigned)yy[1] << 8) | ((unsigned)yy[2] << 16) | ((unsigned)yy[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < n) o[j] = (uint8_t)yy[j];
                }
            }
        }
        const int c0 = x0 >> 1;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (c0 + q < cw) {
                const int bias = (128 << 22) + (1 << 21);
                const int U = (-k.ur * sR[q] - (k.ch - k.ur) * sG[q] + k.ch * sB[q] + bias) >> 22;
                const int V = (k.ch * sR[q] - (k.ch - k.vb) * sG[q] - k.vb * sB[q] + bias) >> 22;
                p.u[(int64_t)by * p.u_stride + c0 + q] = (uint8_t)clampi(U, 0, 255);
                p.v[(int64_t)by * p.v_stride + c0 + q] = (uint8_t)clampi(V, 0, 255);
            }
        }
    }
}

int yuv_blocks(int H, int W) {
    const int64_t threads = (int64_t)((W + 3) >> 2) * ((H + 1) >> 1);
    const int64_t blocks = (threads + 255) >> 8;
    return (int)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

int yuv_common_ok(const char* name, int H, int W, int matrix, int range) {
    OTVM_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: sides are 1 ... 65535, got %d x %d", name, W, H);
    OTVM_REQUIRE(matrix == OTVM_YUV_BT601 || matrix == OTVM_YUV_BT709, "%s: unknown matrix %d", name, matrix);
    OTVM_REQUIRE(range == OTVM_YUV_LIMITED || range == OTVM_YUV_FULL, "%s: unknown range %d", name, range);
    return 0;
}

}  // namespace

extern "C" int otvm_yuv_to_rgb(const otvm_yuv_to_rgb_params* p, void* stream) {
    const char* name = "otvm_yuv_to_rgb";
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (int rc = yuv_common_ok(name, p->H, p->W, p->matrix, p->range)) return rc;
    OTVM_REQUIRE(p->layout >= OTVM_YUV_420P && p->layout <= OTVM_YUV_MONO, "%s: unknown layout %d", name, p->layout);
    OTVM_REQUIRE(p->siting == OTVM_YUV_SITING_LEFT || p->siting == OTVM_YUV_SITING_CENTRE, "%s: unknown siting %d", name, p->siting);
    OTVM_REQUIRE(p->y && p->rgb, "%s: null Y plane / output", name);
    OTVM_REQUIRE(p->y_stride >= p->W, "%s: Y stride %d is shorter than a row of %d", name, p->y_stride, p->W);
    const int cw = (p->W + 1) >> 1;
    const uint8_t* up = p->u;
    const uint8_t* vp = p->v;
    int ustride = p->u_stride, vstride = p->v_stride, cstep = 1;
    if (p->layout == OTVM_YUV_NV12) {
        OTVM_REQUIRE(p->u, "%s: null UV plane", name);
        OTVM_REQUIRE(p->u_stride >= 2 * cw, "%s: UV stride %d is shorter than a row of %d", name, p->u_stride, 2 * cw);
        vp = up + 1;
        vstride = ustride;
        cstep = 2;
    } else if (p->layout != OTVM_YUV_MONO) {
        const int need = p->layout == OTVM_YUV_444P ? p->W : cw;
        OTVM_REQUIRE(p->u && p->v, "%s: null chroma plane", name);
        OTVM_REQUIRE(p->u_stride >= need && p->v_stride >= need, "%s: chroma strides %d, %d are shorter than a row of %d", name,
                     p->u_stride, p->v_stride, need);
    }
    const YuvInv k = kInv[p->matrix][p->range];
    const int yo = p->range == OTVM_YUV_LIMITED ? 16 : 0;
    const dim3 grid(yuv_blocks(p->H, p->W));
    hipStream_t s = (hipStream_t)stream;
    switch (p->layout) {
        case OTVM_YUV_420P:
        case OTVM_YUV_NV12:
            hipLaunchKernelGGL((yuv_to_rgb_kernel<true, true, false>), grid, dim3(256), 0, s, *p, k, yo, up, vp, ustride, vstride, cstep);
            break;
        case OTVM_YUV_422P:
            hipLaunchKernelGGL((yuv_to_rgb_kernel<true, false, false>), grid, dim3(256), 0, s, *p, k, yo, up, vp, ustride, vstride, cstep);
            break;
        case OTVM_YUV_444P:
            hipLaunchKernelGGL((yuv_to_rgb_kernel<false, false, false>), grid, dim3(256), 0, s, *p, k, yo, up, vp, ustride, vstride, cstep);
            break;
        default:
            hipLaunchKernelGGL((yuv_to_rgb_kernel<false, false, true>), grid, dim3(256), 0, s, *p, k, yo, nullptr, nullptr, 0, 0, 1);
            break;
    }
    OTVM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int otvm_rgb_to_yuv420(const otvm_rgb_to_yuv420_params* p, void* stream) {
    const char* name = "otvm_rgb_to_yuv420";
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (int rc = yuv_common_ok(name, p->H, p->W, p->matrix, p->range)) return rc;
    OTVM_REQUIRE(p->img && p->y && p->u && p->v, "%s: null image / plane", name);
    const int cw = (p->W + 1) >> 1;
    OTVM_REQUIRE(p->y_stride >= p->W, "%s: Y stride %d is shorter than a row of %d", name, p->y_stride, p->W);
    OTVM_REQUIRE(p->u_stride >= cw && p->v_stride >= cw, "%s: chroma strides %d, %d are shorter than a row of %d", name, p->u_stride,
                 p->v_stride, cw);
    const YuvFwd k = kFwd[p->matrix][p->range];
    const int yo = p->range == OTVM_YUV_LIMITED ? 16 : 0;
    hipLaunchKernelGGL(rgb_to_yuv420_kernel, dim3(yuv_blocks(p->H, p->W)), dim3(256), 0, (hipStream_t)stream, *p, k, yo);
    OTVM_CHECK_LAUNCH(name);
    return 0;
}
