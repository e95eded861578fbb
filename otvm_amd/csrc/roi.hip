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
//
// The tracking window (otvm_roi_track, otvm_roi_crop_at, otvm_roi_paste_at): the window's origin lives on the device, a row of an
// int32 [T,2] log.  otvm_roi_track derives row t from the box row otvm_trimap_bbox wrote for the neighbouring frame and that
// frame's origin -- two threads, one per axis, integer arithmetic, ordinary stores; otvm_amd/roi.py track_origin is the same policy
// on the host.  The _at forms are the crop and the paste above with (y0, x0) read from such a row: the kernel bodies are shared
// (the window side is never widened, so nothing about alignment depends on the origin), and whatever the row holds is clamped to
// [0, H - h] x [0, W - w] before any address is formed from it.
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

// the origin of a window whose origin lives on the device, clamped into the frame whatever the memory holds
__device__ __forceinline__ int roi_origin_at(const int* __restrict__ origin, int axis, int full, int side) {
    const int v = origin[axis], hi = full - side;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

// a thread takes four consecutive pixels of one WINDOW row; AT: the origin is read from `origin` (a row of the device log)
template <bool VEC, bool AT>
__global__ __launch_bounds__(256) void roi_crop_kernel(const otvm_roi_crop_params p, const int* __restrict__ origin) {
    const int wy0 = AT ? roi_origin_at(origin, 0, p.H, p.h) : p.y0, wx0 = AT ? roi_origin_at(origin, 1, p.W, p.w) : p.x0;
    const int n4 = (p.w + 3) >> 2;
    const int64_t total = (int64_t)p.h * n4, P = (int64_t)p.H * p.W, M = (int64_t)p.h * p.w;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.w - x0 < 4 ? p.w - x0 : 4;
        const int64_t src = (int64_t)(y + wy0) * p.W + (x0 + wx0), dst = (int64_t)y * p.w + x0;
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

// a thread takes four consecutive pixels of one FRAME row; AT: as in the crop
template <bool VEC, bool AT>
__global__ __launch_bounds__(256) void roi_paste_kernel(const otvm_roi_paste_params p, const int* __restrict__ origin) {
    const int wy0 = AT ? roi_origin_at(origin, 0, p.H, p.h) : p.y0, wx0 = AT ? roi_origin_at(origin, 1, p.W, p.w) : p.x0;
    const int n4 = (p.W + 3) >> 2;
    const int64_t total = (int64_t)p.H * n4, N = (int64_t)p.H * p.W, M = (int64_t)p.h * p.w;
    const float s = 1.f / 255.f;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.W - x0 < 4 ? p.W - x0 : 4;
        const int64_t o = (int64_t)y * p.W + x0;
        const bool row_in = y >= wy0 && y < wy0 + p.h;
        // a group that lies inside the window altogether reads nothing of the frame's side
        const bool all_in = row_in && x0 >= wx0 && x0 + n <= wx0 + p.w;
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
            if (j < n && row_in && x >= wx0 && x < wx0 + p.w) {
                const int64_t wi = (int64_t)(y - wy0) * p.w + (x - wx0);
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

namespace {

// thread 0 decides y, thread 1 decides x (otvm_amd/roi.py track_origin, axis by axis).  box: the neighbour's row, its non-background
// box in words 4 .. 7 -- in the neighbour's window when `prev` is given, in the frame otherwise.
__global__ __launch_bounds__(64) void roi_track_kernel(const int* __restrict__ box, const int* __restrict__ prev, int* __restrict__ out,
                                                       int H, int W, int h, int w, int hold) {
    const int a = threadIdx.x;
    if (a >= 2) return;
    const int full = a ? W : H, side = a ? w : h, top = full - side;
    const bool empty = box[6] < box[4] || box[7] < box[5];
    const int64_t lo = box[4 + a], hi = box[6 + a];
    int o = 0;
    bool held = empty;                                     // an empty box keeps the neighbour's origin ((0, 0) without one)
    if (prev) {
        o = roi_origin_at(prev, a, full, side);
        held = held || ((lo >= hold || o == 0) && (side - 1 - hi >= hold || o == top));
    }
    if (!held) {
        // (y0 + y1 + 1) // 2 - h // 2 of the box in frame coordinates; o is an integer, so it leaves the floor as it is
        const int64_t c = o + ((lo + hi + 1) >> 1) - (side >> 1);
        o = (int)(c < 0 ? 0 : (c > top ? top : c));
    }
    out[a] = o;
}

int roi_window_ok(const char* name, int H, int W, int h, int w) {
    OTVM_REQUIRE(roi_side_ok(H) && roi_side_ok(W), "%s: the frame is 1 .. 16383 pixels a side, got %dx%d", name, H, W);
    OTVM_REQUIRE(h >= 1 && w >= 1 && h <= H && w <= W, "%s: a %dx%d window does not fit the %dx%d frame", name, h, w, H, W);
    return 0;
}

int roi_window_at_ok(const char* name, int H, int W, int y0, int x0, int h, int w) {
    OTVM_REQUIRE(roi_side_ok(H) && roi_side_ok(W), "%s: the frame is 1 .. 16383 pixels a side, got %dx%d", name, H, W);
    OTVM_REQUIRE(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && h <= H - y0 && w <= W - x0,
                 "%s: a %dx%d window at (%d, %d) does not lie inside the %dx%d frame", name, h, w, y0, x0, H, W);
    return 0;
}

// origin: NULL = the window is at (p->y0, p->x0); otherwise two device words, and p->y0 / p->x0 are not looked at
int roi_crop_checked(const char* name, const otvm_roi_crop_params* p, const int32_t* origin, bool at, void* stream) {
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (at) {
        OTVM_REQUIRE(origin && ((uintptr_t)origin & 3) == 0, "%s: the origin is two aligned int32 words on the device (y0, x0)", name);
        if (int rc = roi_window_ok(name, p->H, p->W, p->h, p->w)) return rc;
    } else if (int rc = roi_window_at_ok(name, p->H, p->W, p->y0, p->x0, p->h, p->w)) {
        return rc;
    }
    OTVM_REQUIRE(p->frame_out || p->trimap_out || p->labels_out, "%s: no destination", name);
    OTVM_REQUIRE((p->frame || !p->frame_out) && (p->trimap || !p->trimap_out) && (p->labels || !p->labels_out),
                 "%s: a destination without its source", name);
    OTVM_REQUIRE((((uintptr_t)p->trimap | (uintptr_t)p->trimap_out) & 3) == 0, "%s: misaligned trimap", name);
    const bool vec = p->w % 4 == 0 && ((uintptr_t)p->trimap_out & 15) == 0 && (((uintptr_t)p->frame_out | (uintptr_t)p->labels_out) & 3) == 0;
    const dim3 grid(roi_blocks(p->h, p->w));
    hipStream_t s = (hipStream_t)stream;
    if (at) {
        if (vec) hipLaunchKernelGGL((roi_crop_kernel<true, true>), grid, dim3(256), 0, s, *p, origin);
        else hipLaunchKernelGGL((roi_crop_kernel<false, true>), grid, dim3(256), 0, s, *p, origin);
    } else {
        if (vec) hipLaunchKernelGGL((roi_crop_kernel<true, false>), grid, dim3(256), 0, s, *p, nullptr);
        else hipLaunchKernelGGL((roi_crop_kernel<false, false>), grid, dim3(256), 0, s, *p, nullptr);
    }
    OTVM_CHECK_LAUNCH(name);
    return 0;
}

int roi_paste_checked(const char* name, const otvm_roi_paste_params* p, const int32_t* origin, bool at, void* stream) {
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (at) {
        OTVM_REQUIRE(origin && ((uintptr_t)origin & 3) == 0, "%s: the origin is two aligned int32 words on the device (y0, x0)", name);
        if (int rc = roi_window_ok(name, p->H, p->W, p->h, p->w)) return rc;
    } else if (int rc = roi_window_at_ok(name, p->H, p->W, p->y0, p->x0, p->h, p->w)) {
        return rc;
    }
    OTVM_REQUIRE(p->win_alpha && p->win_trimap, "%s: null window alpha or window trimap", name);
    OTVM_REQUIRE(p->alpha || p->alpha_u8 || p->trimap || p->fgr, "%s: no output requested", name);
    OTVM_REQUIRE(!p->fgr || (p->win_fgr && p->frame), "%s: fgr needs the window's F planes and the frame", name);
    OTVM_REQUIRE((((uintptr_t)p->win_alpha | (uintptr_t)p->win_trimap | (uintptr_t)p->win_fgr | (uintptr_t)p->outside | (uintptr_t)p->alpha |
                   (uintptr_t)p->trimap | (uintptr_t)p->fgr) & 3) == 0, "%s: misaligned fp32 plane", name);
    const bool vec = p->W % 4 == 0 && (((uintptr_t)p->outside | (uintptr_t)p->alpha | (uintptr_t)p->trimap | (uintptr_t)p->fgr) & 15) == 0 &&
                     (((uintptr_t)p->alpha_u8 | (uintptr_t)p->frame) & 3) == 0;
    const dim3 grid(roi_blocks(p->H, p->W));
    hipStream_t s = (hipStream_t)stream;
    if (at) {
        if (vec) hipLaunchKernelGGL((roi_paste_kernel<true, true>), grid, dim3(256), 0, s, *p, origin);
        else hipLaunchKernelGGL((roi_paste_kernel<false, true>), grid, dim3(256), 0, s, *p, origin);
    } else {
        if (vec) hipLaunchKernelGGL((roi_paste_kernel<true, false>), grid, dim3(256), 0, s, *p, nullptr);
        else hipLaunchKernelGGL((roi_paste_kernel<false, false>), grid, dim3(256), 0, s, *p, nullptr);
    }
    OTVM_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int otvm_roi_crop(const otvm_roi_crop_params* p, void* stream) { return roi_crop_checked("otvm_roi_crop", p, nullptr, false, stream); }

extern "C" int otvm_roi_paste(const otvm_roi_paste_params* p, void* stream) { return roi_paste_checked("otvm_roi_paste", p, nullptr, false, stream); }

extern "C" int otvm_roi_crop_at(const otvm_roi_crop_params* p, const int32_t* origin, void* stream) {
    return roi_crop_checked("otvm_roi_crop_at", p, origin, true, stream);
}

extern "C" int otvm_roi_paste_at(const otvm_roi_paste_params* p, const int32_t* origin, void* stream) {
    return roi_paste_checked("otvm_roi_paste_at", p, origin, true, stream);
}

extern "C" int otvm_roi_track(const otvm_roi_track_params* p, void* stream) {
    OTVM_REQUIRE(p && p->box && p->out, "otvm_roi_track: null pointer (params, box or out)");
    if (int rc = roi_window_ok("otvm_roi_track", p->H, p->W, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->hold >= 1 && p->hold <= ROI_MAX_SIDE, "otvm_roi_track: hold is 1 .. 16383 pixels, got %d", p->hold);
    OTVM_REQUIRE((((uintptr_t)p->box | (uintptr_t)p->prev | (uintptr_t)p->out) & 3) == 0, "otvm_roi_track: misaligned box, prev or out");
    hipLaunchKernelGGL(roi_track_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p->box, p->prev, p->out, p->H, p->W, p->h, p->w, p->hold);
    OTVM_CHECK_LAUNCH("otvm_roi_track");
    return 0;
}
