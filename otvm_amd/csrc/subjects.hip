// Multi-subject matting (include/otvm_hip.h: otvm_subjects_track, otvm_subjects_crop, otvm_subjects_bbox, otvm_subjects_resolve):
// one clip, S subjects, each followed by a tracking window of its own; the S windows share one size and go through the network
// as one lock-step batch.  The first three are the tracking-window launches of roi.hip over S subjects at once -- the subject is
// the grid's y (crop, bbox) or a thread pair (track) -- so that the launches of a step do not grow with S; the bodies are
// window_ops.h's, the ones roi.hip's single-subject kernels call (and the tests still hold every s against those).  The resolve is
// this file's own pass: one sweep over H x W that pastes the S windows and settles the pixels where they overlap.  Compiled with
// -ffp-contract=off: tests/subjects_ref.py restates the resolve operation by operation, compared bit for bit.
//
// Per-subject buffers come as arrays of OTVM_SUBJECTS_MAX pointers in the params struct (the engine's batched outputs are separate
// tensors); per-subject rows of int32 words as base + s * stride, so that one [S,T,10] log is indexed as it lies.  Whatever an
// origin row holds is clamped to [0, H - h] x [0, W - w] before any address is formed from it (win_origin_at).
#include "window_ops.h"

namespace {

constexpr int SMAX = OTVM_SUBJECTS_MAX;

// thread 2 s decides y of subject s, thread 2 s + 1 its x, on the subject's own rows
__global__ __launch_bounds__(64) void subjects_track_kernel(const otvm_subjects_track_params p) {
    const int t = threadIdx.x;
    if (t >= 2 * p.S) return;
    const int s = t >> 1;
    win_track_axis(p.box_base + (int64_t)s * p.box_stride, p.prev_base ? p.prev_base + (int64_t)s * p.prev_stride : nullptr,
                   p.out_base + (int64_t)s * p.out_stride, t & 1, p.H, p.W, p.h, p.w, p.hold);
}

// blockIdx.y is the subject
template <bool VEC>
__global__ __launch_bounds__(256) void subjects_crop_kernel(const otvm_subjects_crop_params p) {
    const int s = blockIdx.y;
    const int* origin = p.origin_base + (int64_t)s * p.origin_stride;
    win_crop_rows<VEC>(p.frame, p.frame_out[s], p.trimap[s], p.trimap_out[s], nullptr, nullptr, p.H, p.W, p.h, p.w,
                       win_origin_at(origin, 0, p.H, p.h), win_origin_at(origin, 1, p.W, p.w), WIN_FIRST, WIN_STEP);
}

__global__ __launch_bounds__(64) void subjects_bbox_init_kernel(const otvm_subjects_bbox_params p) {
    const int t = threadIdx.x, s = t >> 3, i = t & 7;
    if (s < p.S) (p.out_base + (int64_t)s * p.out_stride)[i] = win_bbox_empty(p.H, p.W, i);
}

// blockIdx.y is the subject; float trimaps only
template <bool VEC>
__global__ __launch_bounds__(256) void subjects_bbox_kernel(const otvm_subjects_bbox_params p) {
    const int s = blockIdx.y;
    win_bbox_reduce<VEC>(p.trimap[s], nullptr, p.H, p.W, p.out_base + (int64_t)s * p.out_stride, WIN_FIRST, WIN_STEP);
}

// a thread takes four consecutive pixels of one FRAME row and all S subjects of them.  The loops over the subjects are unrolled
// to OTVM_SUBJECTS_MAX with a guard, so that the per-subject values stay in registers and the pointer arrays are read at constant
// offsets of the kernel's arguments.
template <bool VEC>
__global__ __launch_bounds__(256) void subjects_resolve_kernel(const otvm_subjects_resolve_params p) {
    const int S = p.S;
    int oy[SMAX], ox[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        oy[s] = 0; ox[s] = 0;
        if (s < S) {
            const int* origin = p.origin_base + (int64_t)s * p.origin_stride;
            oy[s] = win_origin_at(origin, 0, p.H, p.h);
            ox[s] = win_origin_at(origin, 1, p.W, p.w);
        }
    }
    const int n4 = (p.W + 3) >> 2;
    const int64_t total = (int64_t)p.H * n4, N = (int64_t)p.H * p.W, M = (int64_t)p.h * p.w;
    const float sc = 1.f / 255.f;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.W - x0 < 4 ? p.W - x0 : 4;
        const int64_t o = (int64_t)y * p.W + x0;
        // 1. a_s: the window's value inside subject s's window, 0.f outside
        float a[SMAX][4];
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[s][j] = 0.f;
            if (s < S) {
                const bool row_in = y >= oy[s] && y < oy[s] + p.h;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x0 + j;
                    if (j < n && row_in && x >= ox[s] && x < ox[s] + p.w) a[s][j] = p.win_alpha[s][(int64_t)(y - oy[s]) * p.w + (x - ox[s])];
                }
            }
        }
        // 2. the sum in subject order; 3. the rescaling; 8. the union of the unnormalised sum; 9. the owner
        float sum[4], un[4];
        unsigned own[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sum[j] = a[0][j];
#pragma unroll
            for (int s = 1; s < SMAX; ++s)
                if (s < S) sum[j] = sum[j] + a[s][j];
            un[j] = fminf(sum[j], 1.f);
            if (p.normalise && sum[j] > 1.f) {
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (s < S) a[s][j] = a[s][j] / sum[j];
            }
            float best = 0.f;
            own[j] = 255u;
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < S && a[s][j] > best) { best = a[s][j]; own[j] = (unsigned)s; }
        }
        if (VEC) {
            if (p.union_alpha) *reinterpret_cast<f32x4*>(p.union_alpha + o) = f32x4{un[0], un[1], un[2], un[3]};
            if (p.union_u8) {
                *reinterpret_cast<unsigned*>(p.union_u8 + o) =
                    win_byte(un[0]) | (win_byte(un[1]) << 8) | (win_byte(un[2]) << 16) | (win_byte(un[3]) << 24);
            }
            if (p.owner) *reinterpret_cast<unsigned*>(p.owner + o) = own[0] | (own[1] << 8) | (own[2] << 16) | (own[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n) {
                    if (p.union_alpha) p.union_alpha[o + j] = un[j];
                    if (p.union_u8) p.union_u8[o + j] = (uint8_t)win_byte(un[j]);
                    if (p.owner) p.owner[o + j] = (uint8_t)own[j];
                }
            }
        }
        // 4., 5. alpha and its byte per subject
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            if (s < S) {
                const int64_t os = (int64_t)s * N + o;
                if (VEC) {
                    if (p.alpha) *reinterpret_cast<f32x4*>(p.alpha + os) = f32x4{a[s][0], a[s][1], a[s][2], a[s][3]};
                    if (p.alpha_u8) {
                        *reinterpret_cast<unsigned*>(p.alpha_u8 + os) =
                            win_byte(a[s][0]) | (win_byte(a[s][1]) << 8) | (win_byte(a[s][2]) << 16) | (win_byte(a[s][3]) << 24);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < n) {
                            if (p.alpha) p.alpha[os + j] = a[s][j];
                            if (p.alpha_u8) p.alpha_u8[os + j] = (uint8_t)win_byte(a[s][j]);
                        }
                    }
                }
            }
        }
        if (!p.trimap && !p.fgr) continue;
        // 7. outside a window F is the frame's pixel
        float Fo[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { Fo[0][j] = 0.f; Fo[1][j] = 0.f; Fo[2][j] = 0.f; }
        if (p.fgr) {
            unsigned by[12];
            if (VEC) {
                const unsigned* f = reinterpret_cast<const unsigned*>(p.frame + o * 3);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const unsigned wd = f[q];
#pragma unroll
                    for (int j = 0; j < 4; ++j) by[4 * q + j] = (wd >> (8 * j)) & 255u;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) by[j] = j < 3 * n ? (unsigned)p.frame[o * 3 + j] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) Fo[c][j] = (float)by[j * 3 + (p.u8_rgb ? c : 2 - c)] * sc;
        }
        // 6., 7. the trimap and F per subject: the window's inside it, (1, 0, 0) and the frame outside; never rescaled
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            if (s < S) {
                float T[3][4], F[3][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    T[0][j] = 1.f; T[1][j] = 0.f; T[2][j] = 0.f;
                    F[0][j] = Fo[0][j]; F[1][j] = Fo[1][j]; F[2][j] = Fo[2][j];
                }
                const bool row_in = y >= oy[s] && y < oy[s] + p.h;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x0 + j;
                    if (j < n && row_in && x >= ox[s] && x < ox[s] + p.w) {
                        const int64_t wi = (int64_t)(y - oy[s]) * p.w + (x - ox[s]);
                        if (p.trimap) {
#pragma unroll
                            for (int k = 0; k < 3; ++k) T[k][j] = p.win_trimap[s][k * M + wi];
                        }
                        if (p.fgr) {
#pragma unroll
                            for (int k = 0; k < 3; ++k) F[k][j] = p.win_fgr[s][k * M + wi];
                        }
                    }
                }
                const int64_t os = (int64_t)s * 3 * N + o;
                if (VEC) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (p.trimap) *reinterpret_cast<f32x4*>(p.trimap + os + k * N) = f32x4{T[k][0], T[k][1], T[k][2], T[k][3]};
                        if (p.fgr) *reinterpret_cast<f32x4*>(p.fgr + os + k * N) = f32x4{F[k][0], F[k][1], F[k][2], F[k][3]};
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < n) {
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                if (p.trimap) p.trimap[os + k * N + j] = T[k][j];
                                if (p.fgr) p.fgr[os + k * N + j] = F[k][j];
                            }
                        }
                    }
                }
            }
        }
    }
}

int sub_common_ok(const char* name, int S, int H, int W, int h, int w) {
    OTVM_REQUIRE(S >= 1 && S <= SMAX, "%s: 1 .. %d subjects, got %d", name, SMAX, S);
    return win_window_ok(name, H, W, h, w);
}

}  // namespace

extern "C" int otvm_subjects_track(const otvm_subjects_track_params* p, void* stream) {
    OTVM_REQUIRE(p && p->box_base && p->out_base, "otvm_subjects_track: null pointer (params, box_base or out_base)");
    if (int rc = sub_common_ok("otvm_subjects_track", p->S, p->H, p->W, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->hold >= 1 && p->hold <= WIN_MAX_SIDE, "otvm_subjects_track: hold is 1 .. 16383 pixels, got %d", p->hold);
    OTVM_REQUIRE((((uintptr_t)p->box_base | (uintptr_t)p->prev_base | (uintptr_t)p->out_base) & 3) == 0,
                 "otvm_subjects_track: misaligned box_base, prev_base or out_base");
    hipLaunchKernelGGL(subjects_track_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *p);
    OTVM_CHECK_LAUNCH("otvm_subjects_track");
    return 0;
}

extern "C" int otvm_subjects_crop(const otvm_subjects_crop_params* p, void* stream) {
    const char* name = "otvm_subjects_crop";
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (int rc = sub_common_ok(name, p->S, p->H, p->W, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->origin_base && ((uintptr_t)p->origin_base & 3) == 0,
                 "%s: the origins are aligned int32 rows on the device (y0, x0 at origin_base + s * origin_stride)", name);
    int frames = 0, trimaps = 0;
    uintptr_t f32_bits = 0, out16_bits = 0, u8_bits = 0;
    for (int s = 0; s < p->S; ++s) {
        frames += p->frame_out[s] != nullptr;
        trimaps += p->trimap_out[s] != nullptr;
        OTVM_REQUIRE(p->trimap[s] || !p->trimap_out[s], "%s: a destination without its source (trimap of subject %d)", name, s);
        f32_bits |= (uintptr_t)p->trimap[s] | (uintptr_t)p->trimap_out[s];
        out16_bits |= (uintptr_t)p->trimap_out[s];
        u8_bits |= (uintptr_t)p->frame_out[s];
    }
    OTVM_REQUIRE(frames || trimaps, "%s: no destination", name);
    OTVM_REQUIRE((frames == 0 || frames == p->S) && (trimaps == 0 || trimaps == p->S),
                 "%s: a destination is given for every subject or for none", name);
    OTVM_REQUIRE(p->frame || !frames, "%s: a destination without its source (the frame)", name);
    OTVM_REQUIRE((f32_bits & 3) == 0, "%s: misaligned trimap", name);
    otvm_subjects_crop_params q = *p;
    for (int s = p->S; s < SMAX; ++s) { q.frame_out[s] = nullptr; q.trimap[s] = nullptr; q.trimap_out[s] = nullptr; }
    const bool vec = p->w % 4 == 0 && (out16_bits & 15) == 0 && (u8_bits & 3) == 0;
    const dim3 grid(win_blocks(p->h, p->w), (unsigned)p->S);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(subjects_crop_kernel<true>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(subjects_crop_kernel<false>, grid, dim3(256), 0, st, q);
    OTVM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int otvm_subjects_bbox(const otvm_subjects_bbox_params* p, void* stream) {
    const char* name = "otvm_subjects_bbox";
    OTVM_REQUIRE(p && p->out_base, "%s: null pointer (params or out_base)", name);
    OTVM_REQUIRE(p->S >= 1 && p->S <= SMAX, "%s: 1 .. %d subjects, got %d", name, SMAX, p->S);
    if (int rc = win_sides_ok(name, "map", p->H, p->W)) return rc;
    uintptr_t bits = (uintptr_t)p->out_base;
    for (int s = 0; s < p->S; ++s) {
        OTVM_REQUIRE(p->trimap[s], "%s: null trimap of subject %d", name, s);
        bits |= (uintptr_t)p->trimap[s];
    }
    OTVM_REQUIRE((bits & 3) == 0, "%s: misaligned trimap or out_base", name);
    uintptr_t tri_bits = 0;
    for (int s = 0; s < p->S; ++s) tri_bits |= (uintptr_t)p->trimap[s];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(subjects_bbox_init_kernel, dim3(1), dim3(64), 0, st, *p);
    const bool vec = p->W % 4 == 0 && (tri_bits & 15) == 0;
    const dim3 grid(win_blocks(p->H, p->W), (unsigned)p->S);
    if (vec) hipLaunchKernelGGL(subjects_bbox_kernel<true>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(subjects_bbox_kernel<false>, grid, dim3(256), 0, st, *p);
    OTVM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int otvm_subjects_resolve(const otvm_subjects_resolve_params* p, void* stream) {
    const char* name = "otvm_subjects_resolve";
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (int rc = sub_common_ok(name, p->S, p->H, p->W, p->h, p->w)) return rc;
    OTVM_REQUIRE(p->origin_base && ((uintptr_t)p->origin_base & 3) == 0,
                 "%s: the origins are aligned int32 rows on the device (y0, x0 at origin_base + s * origin_stride)", name);
    uintptr_t f32_bits = (uintptr_t)p->alpha | (uintptr_t)p->trimap | (uintptr_t)p->fgr | (uintptr_t)p->union_alpha;
    const uintptr_t out16_bits = f32_bits;
    for (int s = 0; s < p->S; ++s) {
        OTVM_REQUIRE(p->win_alpha[s] && p->win_trimap[s], "%s: null window alpha or window trimap of subject %d", name, s);
        OTVM_REQUIRE(!p->fgr || p->win_fgr[s], "%s: fgr needs the window's F planes of every subject (subject %d has none) and the frame",
                     name, s);
        f32_bits |= (uintptr_t)p->win_alpha[s] | (uintptr_t)p->win_trimap[s] | (uintptr_t)p->win_fgr[s];
    }
    OTVM_REQUIRE(p->alpha || p->alpha_u8 || p->trimap || p->fgr || p->union_alpha || p->union_u8 || p->owner, "%s: no output requested", name);
    OTVM_REQUIRE(!p->fgr || p->frame, "%s: fgr needs the window's F planes of every subject and the frame", name);
    OTVM_REQUIRE((f32_bits & 3) == 0, "%s: misaligned fp32 plane", name);
    const bool vec = p->W % 4 == 0 && (out16_bits & 15) == 0 &&
                     (((uintptr_t)p->alpha_u8 | (uintptr_t)p->union_u8 | (uintptr_t)p->owner | (uintptr_t)p->frame) & 3) == 0;
    const dim3 grid(win_blocks(p->H, p->W));
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(subjects_resolve_kernel<true>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(subjects_resolve_kernel<false>, grid, dim3(256), 0, st, *p);
    OTVM_CHECK_LAUNCH(name);
    return 0;
}
