// Region-of-interest matting (include/otvm_hip.h: otvm_trimap_bbox, otvm_roi_crop, otvm_roi_paste): the boxes of a class map, the
// crop of a frame's inputs to a window, and the paste of the window's results into the frame.  Three memory-bound passes; at
// 1920x1080 the box reads 25 MB (float trimap) or 2 MB (labels), the paste writes up to 60 MB and reads the window, the frame and
// `outside`.  Compiled with -ffp-contract=off: tests/roi_ref.py restates them operation by operation, compared bit for bit.
//
// In all three a thread takes four consecutive pixels of one row of the FULL-SIZE side that is aligned: the source of the box, the
// destination of the crop, the outputs of the paste.  When that width is a multiple of four and the bases are aligned, the four
// pixels move as one 16-byte access per fp32 plane, one dword of label bytes, three dwords of colour bytes; otherwise pixel by
// pixel.  The window side (crop source, paste inputs) starts at any x0 of any W: read element by element, never widened.
//
// The box is a reduction: per thread in registers, per wave through shuffles, per workgroup through LDS, then one integer
// min / max atomic per word and workgroup (at most 2048 workgroups, 8 words) onto words a one-wave kernel set to the empty boxes
// just before on the same stream.  Integer min / max do not depend on the order of arrival.
#include "common.h"

namespace {

typedef float roi_f32x4 __attribute__((ext_vector_type(4)));
constexpr int ROI_MAX_SIDE = 16383;
constexpr int ROI_MAX_BLOCKS = 2048;

__device__ __forceinline__ bool roi_finite(float v) { return fabsf(v) < __builtin_inff(); }

__global__ __launch_bounds__(64) void roi_bbox_init_kernel(int H, int W, int* __restrict__ out) {
    if (threadIdx.x < 8) out[threadIdx.x] = (threadIdx.x & 2) ? -1 : ((threadIdx.x & 1) ? W : H);
}

// words 0, 1, 4, 5 are minima (y0, x0), words 2, 3, 6, 7 maxima (y1, x1)
template <bool VEC>
__global__ __launch_bounds__(256) void roi_bbox_kernel(const float* __restrict__ tri, const uint8_t* __restrict__ lab, int H, int W,
                                                       int* __restrict__ out) {
    __shared__ int part_s[4][8];
    const int n4 = (W + 3) >> 2;
    const int64_t total = (int64_t)H * n4, P = (int64_t)H * W;
    int b[8] = {H, W, -1, -1, H, W, -1, -1};
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = W - x0 < 4 ? W - x0 : 4;
        const int64_t o = (int64_t)y * W + x0;
        unsigned unk = 0, nbg = 0;                         // one bit per pixel of the group
        if (tri) {
            float c[3][4];
            if (VEC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const roi_f32x4 v = *reinterpret_cast<const roi_f32x4*>(tri + k * P + o);
                    c[k][0] = v.x; c[k][1] = v.y; c[k][2] = v.z; c[k][3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) c[k][j] = j < n ? tri[k * P + o + j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool nb = j < n && (c[1][j] > c[0][j] || c[2][j] > c[0][j]);        // max(t1, t2) > t0
                nbg |= (nb ? 1u : 0u) << j;
                unk |= ((nb && c[1][j] >= c[2][j]) ? 1u : 0u) << j;
            }
        } else {
            unsigned v[4];
            if (VEC) {
                const unsigned w = *reinterpret_cast<const unsigned*>(lab + o);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (w >> (8 * j)) & 255u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = j < n ? (unsigned)lab[o + j] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unk |= (v[j] == 1u ? 1u : 0u) << j;
                nbg |= ((v[j] == 1u || v[j] == 2u) ? 1u : 0u) << j;
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned m = s ? nbg : unk;
            if (m) {
                const int lo = x0 + __builtin_ctz(m), hi = x0 + 31 - __builtin_clz(m);
                int* q = b + 4 * s;
                q[0] = y < q[0] ? y : q[0];
                q[1] = lo < q[1] ? lo : q[1];
                q[2] = y > q[2] ? y : q[2];
                q[3] = hi > q[3] ? hi : q[3];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int other = __shfl_xor(b[i], off, 64);
            b[i] = (i & 2) ? (other > b[i] ? other : b[i]) : (other < b[i] ? other : b[i]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) part_s[wave][i] = b[i];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int i = threadIdx.x;
        const bool is_max = (i & 2) != 0;
        int v = part_s[0][i];
        for (int wv = 1; wv < 4; ++wv) {
            const int other = part_s[wv][i];
            v = is_max ? (other > v ? other : v) : (other < v ? other : v);
        }
        // (a workgroup that found nothing holds the empty box: nothing to merge)
        if (is_max) { if (v >= 0) atomicMax(out + i, v); }
        else        { if (v < ((i & 1) ? W : H)) atomicMin(out + i, v); }
    }
}

// a thread takes four consecutive pixels of one WINDOW row
template <bool VEC>
__global__ __launch_bounds__(256) void roi_crop_kernel(const otvm_roi_crop_params p) {
    const int n4 = (p.w + 3) >> 2;
    const int64_t total = (int64_t)p.h * n4, P = (int64_t)p.H * p.W, M = (int64_t)p.h * p.w;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.w - x0 < 4 ? p.w - x0 : 4;
        const int64_t src = (int64_t)(y + p.y0) * p.W + (x0 + p.x0), dst = (int64_t)y * p.w + x0;
        if (p.frame_out) {
            unsigned by[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) by[j] = j < 3 * n ? (unsigned)p.frame[src * 3 + j] : 0u;
            if (VEC) {
                unsigned* d = reinterpret_cast<unsigned*>(p.frame_out + dst * 3);
#pragma unroll
                for (int q = 0; q < 3; ++q) d[q] = by[4 * q] | (by[4 * q + 1] << 8) | (by[4 * q + 2] << 16) | (by[4 * q + 3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < 3 * n) p.frame_out[dst * 3 + j] = (uint8_t)by[j];
            }
        }
        if (p.trimap_out) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = j < n ? p.trimap[k * P + src + j] : 0.f;
                if (VEC) {
                    *reinterpret_cast<roi_f32x4*>(p.trimap_out + k * M + dst) = roi_f32x4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < n) p.trimap_out[k * M + dst + j] = v[j];
                }
            }
        }
        if (p.labels_out) {
            unsigned v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = j < n ? (unsigned)p.labels[src + j] : 0u;
            if (VEC) {
                *reinterpret_cast<unsigned*>(p.labels_out + dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) p.labels_out[dst + j] = (uint8_t)v[j];
            }
        }
    }
}

// a thread takes four consecutive pixels of one FRAME row
template <bool VEC>
__global__ __launch_bounds__(256) void roi_paste_kernel(const otvm_roi_paste_params p) {
    const int n4 = (p.W + 3) >> 2;
    const int64_t total = (int64_t)p.H * n4, N = (int64_t)p.H * p.W, M = (int64_t)p.h * p.w;
    const float s = 1.f / 255.f;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.W - x0 < 4 ? p.W - x0 : 4;
        const int64_t o = (int64_t)y * p.W + x0;
        const bool row_in = y >= p.y0 && y < p.y0 + p.h;
        // a group that lies inside the window altogether reads nothing of the frame's side
        const bool all_in = row_in && x0 >= p.x0 && x0 + n <= p.x0 + p.w;
        float a[4], T[3][4], F[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            T[0][j] = 1.f; T[1][j] = 0.f; T[2][j] = 0.f;
            F[0][j] = 0.f; F[1][j] = 0.f; F[2][j] = 0.f;
        }
        if (!all_in) {
            if (p.outside) {
                if (VEC) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const roi_f32x4 v = *reinterpret_cast<const roi_f32x4*>(p.outside + k * N + o);
                        T[k][0] = v.x; T[k][1] = v.y; T[k][2] = v.z; T[k][3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < n) T[k][j] = p.outside[k * N + o + j];
                }
            }
            if (p.fgr) {
                unsigned by[12];
                if (VEC) {
                    const unsigned* f = reinterpret_cast<const unsigned*>(p.frame + o * 3);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const unsigned w = f[q];
#pragma unroll
                        for (int j = 0; j < 4; ++j) by[4 * q + j] = (w >> (8 * j)) & 255u;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 12; ++j) by[j] = j < 3 * n ? (unsigned)p.frame[o * 3 + j] : 0u;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) F[c][j] = (float)by[j * 3 + (p.u8_rgb ? c : 2 - c)] * s;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            a[j] = T[2][j] == 1.f ? 1.f : 0.f;
            if (j < n && row_in && x >= p.x0 && x < p.x0 + p.w) {
                const int64_t wi = (int64_t)(y - p.y0) * p.w + (x - p.x0);
                a[j] = p.win_alpha[wi];
#pragma unroll
                for (int k = 0; k < 3; ++k) T[k][j] = p.win_trimap[k * M + wi];
                if (p.fgr) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) F[k][j] = p.win_fgr[k * M + wi];
                }
            }
        }
        unsigned q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = fminf(fmaxf(truncf(a[j] * 255.f), 0.f), 255.f);
            q[j] = roi_finite(a[j]) ? (unsigned)(int)v : 0u;
        }
        if (VEC) {
            if (p.alpha) *reinterpret_cast<roi_f32x4*>(p.alpha + o) = roi_f32x4{a[0], a[1], a[2], a[3]};
            if (p.alpha_u8) *reinterpret_cast<unsigned*>(p.alpha_u8 + o) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (p.trimap) *reinterpret_cast<roi_f32x4*>(p.trimap + k * N + o) = roi_f32x4{T[k][0], T[k][1], T[k][2], T[k][3]};
                if (p.fgr) *reinterpret_cast<roi_f32x4*>(p.fgr + k * N + o) = roi_f32x4{F[k][0], F[k][1], F[k][2], F[k][3]};
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n) {
                    if (p.alpha) p.alpha[o + j] = a[j];
                    if (p.alpha_u8) p.alpha_u8[o + j] = (uint8_t)q[j];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (p.trimap) p.trimap[k * N + o + j] = T[k][j];
                        if (p.fgr) p.fgr[k * N + o + j] = F[k][j];
                    }
                }
            }
        }
    }
}

bool roi_side_ok(int v) { return v >= 1 && v <= ROI_MAX_SIDE; }

unsigned roi_blocks(int64_t rows, int width) {
    const int64_t b = (rows * ((width + 3) / 4) + 255) / 256;
    return (unsigned)(b > ROI_MAX_BLOCKS ? ROI_MAX_BLOCKS : b);
}

}  // namespace

extern "C" int otvm_trimap_bbox(const otvm_roi_bbox_params* p, void* stream) {
    OTVM_REQUIRE(p && p->out, "otvm_trimap_bbox: null pointer (params or out)");
    OTVM_REQUIRE((p->trimap != nullptr) != (p->labels != nullptr),
                 "otvm_trimap_bbox: exactly one source is given, a float trimap [3,H,W] or a uint8 label map [H,W]");
    OTVM_REQUIRE(roi_side_ok(p->H) && roi_side_ok(p->W), "otvm_trimap_bbox: the map is 1 .. 16383 pixels a side, got %dx%d", p->H, p->W);
    OTVM_REQUIRE((((uintptr_t)p->trimap | (uintptr_t)p->out) & 3) == 0, "otvm_trimap_bbox: misaligned trimap or out");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(roi_bbox_init_kernel, dim3(1), dim3(64), 0, s, p->H, p->W, p->out);
    const bool vec = p->W % 4 == 0 && ((uintptr_t)p->trimap & 15) == 0 && ((uintptr_t)p->labels & 3) == 0;
    const dim3 grid(roi_blocks(p->H, p->W));
    if (vec) hipLaunchKernelGGL(roi_bbox_kernel<true>, grid, dim3(256), 0, s, p->trimap, p->labels, p->H, p->W, p->out);
    else hipLaunchKernelGGL(roi_bbox_kernel<false>, grid, dim3(256), 0, s, p->trimap, p->labels, p->H, p->W, p->out);
    OTVM_CHECK_LAUNCH("otvm_trimap_bbox");
    return 0;
}

#define ROI_REQUIRE_WINDOW(name, p)                                                                                                  \
    OTVM_REQUIRE(roi_side_ok((p)->H) && roi_side_ok((p)->W), name ": the frame is 1 .. 16383 pixels a side, got %dx%d", (p)->H, (p)->W); \
    OTVM_REQUIRE((p)->h >= 1 && (p)->w >= 1 && (p)->y0 >= 0 && (p)->x0 >= 0 && (p)->h <= (p)->H - (p)->y0 && (p)->w <= (p)->W - (p)->x0, \
                 name ": a %dx%d window at (%d, %d) does not lie inside the %dx%d frame", (p)->h, (p)->w, (p)->y0, (p)->x0, (p)->H, (p)->W)

extern "C" int otvm_roi_crop(const otvm_roi_crop_params* p, void* stream) {
    OTVM_REQUIRE(p, "otvm_roi_crop: null parameters");
    ROI_REQUIRE_WINDOW("otvm_roi_crop", p);
    OTVM_REQUIRE(p->frame_out || p->trimap_out || p->labels_out, "otvm_roi_crop: no destination");
    OTVM_REQUIRE((p->frame || !p->frame_out) && (p->trimap || !p->trimap_out) && (p->labels || !p->labels_out),
                 "otvm_roi_crop: a destination without its source");
    OTVM_REQUIRE((((uintptr_t)p->trimap | (uintptr_t)p->trimap_out) & 3) == 0, "otvm_roi_crop: misaligned trimap");
    const bool vec = p->w % 4 == 0 && ((uintptr_t)p->trimap_out & 15) == 0 && (((uintptr_t)p->frame_out | (uintptr_t)p->labels_out) & 3) == 0;
    const dim3 grid(roi_blocks(p->h, p->w));
    if (vec) hipLaunchKernelGGL(roi_crop_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(roi_crop_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    OTVM_CHECK_LAUNCH("otvm_roi_crop");
    return 0;
}

extern "C" int otvm_roi_paste(const otvm_roi_paste_params* p, void* stream) {
    OTVM_REQUIRE(p, "otvm_roi_paste: null parameters");
    ROI_REQUIRE_WINDOW("otvm_roi_paste", p);
    OTVM_REQUIRE(p->win_alpha && p->win_trimap, "otvm_roi_paste: null window alpha or window trimap");
    OTVM_REQUIRE(p->alpha || p->alpha_u8 || p->trimap || p->fgr, "otvm_roi_paste: no output requested");
    OTVM_REQUIRE(!p->fgr || (p->win_fgr && p->frame), "otvm_roi_paste: fgr needs the window's F planes and the frame");
    OTVM_REQUIRE((((uintptr_t)p->win_alpha | (uintptr_t)p->win_trimap | (uintptr_t)p->win_fgr | (uintptr_t)p->outside | (uintptr_t)p->alpha |
                   (uintptr_t)p->trimap | (uintptr_t)p->fgr) & 3) == 0, "otvm_roi_paste: misaligned fp32 plane");
    const bool vec = p->W % 4 == 0 && (((uintptr_t)p->outside | (uintptr_t)p->alpha | (uintptr_t)p->trimap | (uintptr_t)p->fgr) & 15) == 0 &&
                     (((uintptr_t)p->alpha_u8 | (uintptr_t)p->frame) & 3) == 0;
    const dim3 grid(roi_blocks(p->H, p->W));
    if (vec) hipLaunchKernelGGL(roi_paste_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(roi_paste_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    OTVM_CHECK_LAUNCH("otvm_roi_paste");
    return 0;
}
