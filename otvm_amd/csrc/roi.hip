// Region-of-interest matting (include/otvm_hip.h: otvm_trimap_bbox, otvm_roi_crop, otvm_roi_paste): the boxes of a class map, the
// crop of a frame's inputs to a window, and the paste of the window's results into the frame.  Three memory-bound passes; at
// 1920x1080 the box reads 25 MB (float trimap) or 2 MB (labels), the paste writes up to 60 MB and reads the window, the frame and
// `outside`.  Compiled with -ffp-contract=off: tests/roi_ref.py restates them operation by operation, compared bit for bit.
// The access pattern, the box reduction, the crop's rows and the tracking policy are window_ops.h's, shared with subjects.hip;
// what is this file's own is the paste, the static window (an origin in the params) and the label maps.
//
// The tracking window (otvm_roi_track, otvm_roi_crop_at, otvm_roi_paste_at): the window's origin lives on the device, a row of an
// int32 [T,2] log.  otvm_roi_track derives row t from the box row otvm_trimap_bbox wrote for the neighbouring frame and that
// frame's origin -- two threads, one per axis, integer arithmetic, ordinary stores; otvm_amd/roi.py track_origin is the same policy
// on the host.  The _at forms are the crop and the paste above with (y0, x0) read from such a row: one kernel body serves both,
// and whatever the row holds is clamped to [0, H - h] x [0, W - w] before any address is formed from it.
#include "window_ops.h"

namespace {

__global__ __launch_bounds__(64) void roi_bbox_init_kernel(int H, int W, int* __restrict__ out) {
    if (threadIdx.x < 8) out[threadIdx.x] = win_bbox_empty(H, W, threadIdx.x);
}

template <bool VEC>
__global__ __launch_bounds__(256) void roi_bbox_kernel(const float* __restrict__ tri, const uint8_t* __restrict__ lab, int H, int W,
                                                       int* __restrict__ out) {
    win_bbox_reduce<VEC>(tri, lab, H, W, out, WIN_FIRST, WIN_STEP);
}

// AT: the origin is read from `origin` (a row of the device log)
template <bool VEC, bool AT>
__global__ __launch_bounds__(256) void roi_crop_kernel(const otvm_roi_crop_params p, const int* __restrict__ origin) {
    const int wy0 = AT ? win_origin_at(origin, 0, p.H, p.h) : p.y0, wx0 = AT ? win_origin_at(origin, 1, p.W, p.w) : p.x0;
    win_crop_rows<VEC>(p.frame, p.frame_out, p.trimap, p.trimap_out, p.labels, p.labels_out, p.H, p.W, p.h, p.w, wy0, wx0,
                       WIN_FIRST, WIN_STEP);
}

// a thread takes four consecutive pixels of one FRAME row; AT: as in the crop
template <bool VEC, bool AT>
__global__ __launch_bounds__(256) void roi_paste_kernel(const otvm_roi_paste_params p, const int* __restrict__ origin) {
    const int wy0 = AT ? win_origin_at(origin, 0, p.H, p.h) : p.y0, wx0 = AT ? win_origin_at(origin, 1, p.W, p.w) : p.x0;
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
                        const f32x4 v = *reinterpret_cast<const f32x4*>(p.outside + k * N + o);
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
        for (int j = 0; j < 4; ++j) q[j] = win_byte(a[j]);
        if (VEC) {
            if (p.alpha) *reinterpret_cast<f32x4*>(p.alpha + o) = f32x4{a[0], a[1], a[2], a[3]};
            if (p.alpha_u8) *reinterpret_cast<unsigned*>(p.alpha_u8 + o) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (p.trimap) *reinterpret_cast<f32x4*>(p.trimap + k * N + o) = f32x4{T[k][0], T[k][1], T[k][2], T[k][3]};
                if (p.fgr) *reinterpret_cast<f32x4*>(p.fgr + k * N + o) = f32x4{F[k][0], F[k][1], F[k][2], F[k][3]};
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

// thread 0 decides y, thread 1 decides x
__global__ __launch_bounds__(64) void roi_track_kernel(const int* __restrict__ box, const int* __restrict__ prev, int* __restrict__ out,
                                                       int H, int W, int h, int w, int hold) {
    if (threadIdx.x < 2) win_track_axis(box, prev, out, threadIdx.x, H, W, h, w, hold);
}

int roi_window_at_ok(const char* name, int H, int W, int y0, int x0, int h, int w) {
    if (int rc = win_sides_ok(name, "frame", H, W)) return rc;
    OTVM_REQUIRE(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && h <= H - y0 && w <= W - x0,
                 "%s: a %dx%d window at (%d, %d) does not lie inside the %dx%d frame", name, h, w, y0, x0, H, W);
    return 0;
}

// origin: NULL = the window is at (p->y0, p->x0); otherwise two device words, and p->y0 / p->x0 are not looked at
int roi_crop_checked(const char* name, const otvm_roi_crop_params* p, const int32_t* origin, bool at, void* stream) {
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (at) {
        OTVM_REQUIRE(origin && ((uintptr_t)origin & 3) == 0, "%s: the origin is two aligned int32 words on the device (y0, x0)", name);
        if (int rc = win_window_ok(name, p->H, p->W, p->h, p->w)) return rc;
    } else if (int rc = roi_window_at_ok(name, p->H, p->W, p->y0, p->x0, p->h, p->w)) {
        return rc;
    }
    OTVM_REQUIRE(p->frame_out || p->trimap_out || p->labels_out, "%s: no destination", name);
    OTVM_REQUIRE((p->frame || !p->frame_out) && (p->trimap || !p->trimap_out) && (p->labels || !p->labels_out),
                 "%s: a destination without its source", name);
    OTVM_REQUIRE((((uintptr_t)p->trimap | (uintptr_t)p->trimap_out) & 3) == 0, "%s: misaligned trimap", name);
    const bool vec = p->w % 4 == 0 && ((uintptr_t)p->trimap_out & 15) == 0 && (((uintptr_t)p->frame_out | (uintptr_t)p->labels_out) & 3) == 0;
    const dim3 grid(win_blocks(p->h, p->w));
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
        if (int rc = win_window_ok(name, p->H, p->W, p->h, p->w)) return rc;
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
    const dim3 grid(win_blocks(p->H, p->W));
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

extern "C" int otvm_trimap_bbox(const otvm_roi_bbox_params* p, void* stream) {
    OTVM_REQUIRE(p && p->out, "otvm_trimap_bbox: null pointer (params or out)");
    OTVM_REQUIRE((p->trimap != nullptr) != (p->labels != nullptr),
                 "otvm_trimap_bbox: exactly one source is given, a float trimap [3,H,W] or a uint8 label map [H,W]");
    if (int rc = win_sides_ok("otvm_trimap_bbox", "map", p->H, p->W)) return rc;
    OTVM_REQUIRE((((uintptr_t)p->trimap | (uintptr_t)p->out) & 3) == 0, "otvm_trimap_bbox: misaligned trimap or out");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(roi_bbox_init_kernel, dim3(1), dim3(64), 0, s, p->H, p->W, p->out);
    const bool vec = p->W % 4 == 0 && ((uintptr_t)p->trimap & 15) == 0 && ((uintptr_t)p->labels & 3) == 0;
    const dim3 grid(win_blocks(p->H, p->W));
    if (vec) hipLaunchKernelGGL(roi_bbox_kernel<true>, grid, dim3(256), 0, s, p->trimap, p->labels, p->H, p->W, p->out);
    else hipLaunchKernelGGL(roi_bbox_kernel<false>, grid, dim3(256), 0, s, p->trimap, p->labels, p->H, p->W, p->out);
    OTVM_CHECK_LAUNCH("otvm_trimap_bbox");
    return 0;
}

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
    if (int rc = win_window_ok("otvm_roi_track", p->H, p->W, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->hold >= 1 && p->hold <= WIN_MAX_SIDE, "otvm_roi_track: hold is 1 .. 16383 pixels, got %d", p->hold);
    OTVM_REQUIRE((((uintptr_t)p->box | (uintptr_t)p->prev | (uintptr_t)p->out) & 3) == 0, "otvm_roi_track: misaligned box, prev or out");
    hipLaunchKernelGGL(roi_track_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p->box, p->prev, p->out, p->H, p->W, p->h, p->w, p->hold);
    OTVM_CHECK_LAUNCH("otvm_roi_track");
    return 0;
}
