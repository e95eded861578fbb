// The window kernels' shared bodies: roi.hip (one window) and subjects.hip (S windows of one size) are thin kernels round them, so
// that the hold rule, the box rule, the byte quantiser and the origin clamp are written once.  Both are compiled with
// -ffp-contract=off; everything here is forced inline, and a pointer carries `__restrict__` only where the kernel's own says so.
//
// The access pattern of every pass: a thread takes four consecutive pixels of one row of the FULL-SIZE side that is aligned -- the
// source of the box, the destination of the crop, the outputs of the paste and of the resolve.  When that width is a multiple of
// four and the bases are aligned (VEC), the four pixels move as one 16-byte access per fp32 plane, one dword of label bytes, three
// dwords of colour bytes; otherwise pixel by pixel.  The window side (crop source, paste and resolve inputs) starts at any x0 of
// any W: read element by element, never widened, so nothing about alignment depends on a window's origin.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int WIN_MAX_SIDE = 16383;
constexpr int WIN_MAX_BLOCKS = 2048;

// ---- host side: limits, grids and the refusals every entry point shares (`name`: the entry point, so each keeps its message)
static inline bool win_side_ok(int v) { return v >= 1 && v <= WIN_MAX_SIDE; }

// workgroups of 256 threads over rows x ceil(width / 4) groups of four pixels; the kernels stride over what is left
static inline unsigned win_blocks(int64_t rows, int width) {
    const int64_t b = (rows * ((width + 3) / 4) + 255) / 256;
    return (unsigned)(b > WIN_MAX_BLOCKS ? WIN_MAX_BLOCKS : b);
}

// what: "frame" or "map"
static inline int win_sides_ok(const char* name, const char* what, int H, int W) {
    OTVM_REQUIRE(win_side_ok(H) && win_side_ok(W), "%s: the %s is 1 .. 16383 pixels a side, got %dx%d", name, what, H, W);
    return 0;
}

// an h x w window whose origin lives on the device: all the host can say is that it fits the frame
static inline int win_window_ok(const char* name, int H, int W, int h, int w) {
    if (int rc = win_sides_ok(name, "frame", H, W)) return rc;
    OTVM_REQUIRE(h >= 1 && w >= 1 && h <= H && w <= W, "%s: a %dx%d window does not fit the %dx%d frame", name, h, w, H, W);
    return 0;
}

// The grid-stride loops of the bodies below run t = first, first + step, ... : the thread's index in the grid and the grid's size in
// threads.  The __global__ function passes them (WIN_FIRST, WIN_STEP): only there does the compiler fold blockDim.x to the uniform
// workgroup size; read inside an inlined body it costs a dependent load and a select before the loop (profiles/
// refactor_window_ops_isa_diff.txt).
#define WIN_FIRST ((int64_t)blockIdx.x * blockDim.x + threadIdx.x)
#define WIN_STEP ((int64_t)gridDim.x * blockDim.x)

// ---- the origin, the quantiser
// the origin of a window whose origin lives on the device, clamped into the frame whatever the memory holds
__device__ __forceinline__ int win_origin_at(const int* __restrict__ origin, int axis, int full, int side) {
    const int v = origin[axis], hi = full - side;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

__device__ __forceinline__ bool win_finite(float v) { return fabsf(v) < __builtin_inff(); }

// alpha as a byte: trunc(a * 255) clamped to 0 .. 255, 0 for what is not finite
__device__ __forceinline__ unsigned win_byte(float a) {
    const float v = fminf(fmaxf(truncf(a * 255.f), 0.f), 255.f);
    return win_finite(a) ? (unsigned)(int)v : 0u;
}

// ---- the tracking policy, one axis (0: y, 1: x) of one window: otvm_amd/roi.py track_origin, axis by axis.  box: the neighbour's
// row, its non-background box in words 4 .. 7 -- in the neighbour's window when `prev` (its origin) is given, in the frame otherwise.
__device__ __forceinline__ void win_track_axis(const int* box, const int* prev, int* out, int a, int H, int W, int h, int w, int hold) {
    const int full = a ? W : H, side = a ? w : h, top = full - side;
    const bool empty = box[6] < box[4] || box[7] < box[5];
    const int64_t lo = box[4 + a], hi = box[6 + a];
    int o = 0;
    bool held = empty;                                     // an empty box keeps the neighbour's origin ((0, 0) without one)
    if (prev) {
        o = win_origin_at(prev, a, full, side);
        held = held || ((lo >= hold || o == 0) && (side - 1 - hi >= hold || o == top));
    }
    if (!held) {
        // (y0 + y1 + 1) // 2 - h // 2 of the box in frame coordinates; o is an integer, so it leaves the floor as it is
        const int64_t c = o + ((lo + hi + 1) >> 1) - (side >> 1);
        o = (int)(c < 0 ? 0 : (c > top ? top : c));
    }
    out[a] = o;
}

// ---- the boxes of a class map.  A reduction: per thread in registers, per wave through shuffles, per workgroup through LDS, then
// one integer min / max atomic per word and workgroup (at most 2048 workgroups, 8 words) onto words that were set to the
// empty boxes (win_bbox_empty) just before on the same stream.  Integer min / max do not depend on the order of arrival.
// words 0, 1, 4, 5 are minima (y0, x0), words 2, 3, 6, 7 maxima (y1, x1)
__device__ __forceinline__ int win_bbox_empty(int H, int W, unsigned i) { return (i & 2) ? -1 : ((i & 1) ? W : H); }

// tri: a float trimap [3,H,W], or nullptr and then lab: a uint8 label map [H,W].  Called by all 256 threads of the workgroup.
template <bool VEC>
__device__ __forceinline__ void win_bbox_reduce(const float* tri, const uint8_t* lab, int H, int W, int* out, int64_t first, int64_t step) {
    __shared__ int part_s[4][8];
    const int n4 = (W + 3) >> 2;
    const int64_t total = (int64_t)H * n4, P = (int64_t)H * W;
    int b[8] = {H, W, -1, -1, H, W, -1, -1};
    for (int64_t t = first; t < total; t += step) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = W - x0 < 4 ? W - x0 : 4;
        const int64_t o = (int64_t)y * W + x0;
        unsigned unk = 0, nbg = 0;                         // one bit per pixel of the group
        if (tri) {
            float c[3][4];
            if (VEC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(tri + k * P + o);
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

// ---- the crop: a thread takes four consecutive pixels of one WINDOW row, the h x w window at (wy0, wx0) of an H x W frame.  Every
// destination that is given is filled from its source: frame uint8 [.,.,3], trimap fp32 [3,.,.], labels uint8 [.,.].
template <bool VEC>
__device__ __forceinline__ void win_crop_rows(const uint8_t* frame, uint8_t* frame_out, const float* trimap, float* trimap_out,
                                              const uint8_t* labels, uint8_t* labels_out, int H, int W, int h, int w, int wy0, int wx0,
                                              int64_t first, int64_t step) {
    const int n4 = (w + 3) >> 2;
    const int64_t total = (int64_t)h * n4, P = (int64_t)H * W, M = (int64_t)h * w;
    for (int64_t t = first; t < total; t += step) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = w - x0 < 4 ? w - x0 : 4;
        const int64_t src = (int64_t)(y + wy0) * W + (x0 + wx0), dst = (int64_t)y * w + x0;
        if (frame_out) {
            unsigned by[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) by[j] = j < 3 * n ? (unsigned)frame[src * 3 + j] : 0u;
            if (VEC) {
                unsigned* d = reinterpret_cast<unsigned*>(frame_out + dst * 3);
#pragma unroll
                for (int q = 0; q < 3; ++q) d[q] = by[4 * q] | (by[4 * q + 1] << 8) | (by[4 * q + 2] << 16) | (by[4 * q + 3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < 3 * n) frame_out[dst * 3 + j] = (uint8_t)by[j];
            }
        }
        if (trimap_out) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = j < n ? trimap[k * P + src + j] : 0.f;
                if (VEC) {
                    *reinterpret_cast<f32x4*>(trimap_out + k * M + dst) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < n) trimap_out[k * M + dst + j] = v[j];
                }
            }
        }
        if (labels_out) {
            unsigned v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = j < n ? (unsigned)labels[src + j] : 0u;
            if (VEC) {
                *reinterpret_cast<unsigned*>(labels_out + dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) labels_out[dst + j] = (uint8_t)v[j];
            }
        }
    }
}
