// Temporal stabilisation of alpha (include/otvm_hip.h: otvm_luma_u8, otvm_temporal_blend): a causal, one-frame-state,
// motion-compensated recursive filter.  The previous STABILISED alpha and the previous grey frame are sampled bilinearly where
// the flow (otvm_optflow_farneback of this frame's grey against the previous one's) points; the photometric residual, the change
// of alpha and the trimap's unknown class weigh the blend.  Compiled with -ffp-contract=off: tests/temporal_ref.py restates the
// arithmetic operation by operation and the outputs are compared bit for bit.  No atomics, no LDS.
//
// Both kernels are memory-bound.  The blend moves 4 (alpha) + 8 (flow) + 1 (grey) + 4 + 1 (out, byte) = 18 B per pixel in
// streams, 12 B of trimap when there is one, and gathers 4 x (4 + 1) B of the previous planes, which lie within a few pixels of
// the thread's own position and stay in L2; the two taps of a row are one load (a float pair, a byte pair), so a pixel issues
// four gathers, and a trimap at the frame's own resolution comes as three 16-byte loads per group.  A thread takes four
// consecutive pixels of a row: with W a multiple of four (and 16-byte aligned bases) alpha is one 16-byte load, the flow two, the
// grey bytes one dword, and out / out_u8 leave as one 16-byte store and one dword.  Otherwise, and for the last one to three
// pixels of a row, the same values move pixel by pixel.
// The luma kernel reads 3 B and writes 1 B per pixel: a thread takes sixteen consecutive pixels (the image is one flat run of
// pixels), three 16-byte loads and one 16-byte store; the last N % 16 pixels, or unaligned bases, go pixel by pixel.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }      // false for NaN and +-inf

// OpenCV's BGR2GRAY on bytes: (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 (the weights sum to 16384: 255 stays 255)
__device__ __forceinline__ unsigned luma_of(unsigned c0, unsigned c1, unsigned c2, int u8_rgb) {
    const unsigned b = u8_rgb ? c2 : c0, r = u8_rgb ? c0 : c2;
    return (b * 1868u + c1 * 9617u + r * 4899u + 8192u) >> 14;
}

__global__ __launch_bounds__(256) void luma_u8_kernel(const uint8_t* __restrict__ img, const int64_t N, const int u8_rgb,
                                                      uint8_t* __restrict__ grey, const int vec) {
    const int64_t groups = (N + 15) >> 4;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p0 = g << 4;
        if (vec && p0 + 16 <= N) {
            const u32x4* src = reinterpret_cast<const u32x4*>(img + p0 * 3);
            const u32x4 a = src[0], b = src[1], c = src[2];
            const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = 3 * k;
                const unsigned c0 = (w[i >> 2] >> (8 * (i & 3))) & 255u;
                const unsigned c1 = (w[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 255u;
                const unsigned c2 = (w[(i + 2) >> 2] >> (8 * ((i + 2) & 3))) & 255u;
                o[k >> 2] |= luma_of(c0, c1, c2, u8_rgb) << (8 * (k & 3));
            }
            *reinterpret_cast<u32x4*>(grey + p0) = u32x4{o[0], o[1], o[2], o[3]};
        } else {
            const int64_t p1 = p0 + 16 < N ? p0 + 16 : N;
            for (int64_t p = p0; p < p1; ++p)
                grey[p] = (uint8_t)luma_of(img[p * 3], img[p * 3 + 1], img[p * 3 + 2], u8_rgb);
        }
    }
}

// fmaxf(0, v) / the clamp to [0,1] as selects: the same values, and no choice left for -0.0 (gives +0.0) or NaN (gives 0)
__device__ __forceinline__ float ramp0(float v) { return v > 0.f ? v : 0.f; }
__device__ __forceinline__ float clamp01(float v) {
    const float lo = v > 0.f ? v : 0.f;
    return lo < 1.f ? lo : 1.f;
}

// two horizontally adjacent taps in one load: a float pair at any dword, a byte pair at any byte
typedef float f32x2_any __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned short u16_any __attribute__((aligned(1)));

// the trimap's gate at (x, y): numpy's first-max argmax == 1 (the unknown class); NaN closes the gate
__device__ __forceinline__ float gate_of(float t0, float t1, float t2) { return (t1 > t0 && t1 >= t2) ? 1.f : 0.f; }
__device__ __forceinline__ float gate_at(const otvm_temporal_params& p, int x, int y) {
    const int64_t plane = (int64_t)p.th * p.tw;
    const int64_t ti = (int64_t)min(y / p.tri_scale, p.th - 1) * p.tw + min(x / p.tri_scale, p.tw - 1);
    return gate_of(p.tri[ti], p.tri[plane + ti], p.tri[2 * plane + ti]);
}

// One pixel.  a = this frame's raw alpha at (x, y); g = its grey byte; (dx, dy) = the flow to the previous frame; gate = the
// trimap's (1 without one).
__device__ __forceinline__ float blend_pixel(const otvm_temporal_params& p, int x, int y, float a, unsigned g, float dx, float dy,
                                             float gate) {
    float w = 0.f, sw = 0.f;
    if (p.prev) {                                                 // (uniform) NULL: the first frame of a clip, w = 0 everywhere
        const float sx = (float)x + dx, sy = (float)y + dy;
        const bool ok = sx >= 0.f && sx <= (float)(p.W - 1) && sy >= 0.f && sy <= (float)(p.H - 1);      // NaN, +-inf: false
        if (ok) {
            const float fx0 = floorf(sx), fy0 = floorf(sy);
            const float fx = sx - fx0, fy = sy - fy0;
            // (the min only matters beyond W, H = 2^24, where (float)(W - 1) may round up: the gathers stay inside the planes)
            const int x0 = min((int)fx0, p.W - 1), y0 = min((int)fy0, p.H - 1);
            const int y1 = min(y0 + 1, p.H - 1);                  // (x1 = min(x0 + 1, W - 1): the pair below)
            const int64_t r0 = (int64_t)y0 * p.W, r1 = (int64_t)y1 * p.W;
            const float ofx = 1.f - fx, ofy = 1.f - fy;
            float v00, v01, v10, v11, g00, g01, g10, g11;
            if (p.W > 1) {                                        // (uniform) the taps x0, x1 of a row come as one pair
                // the pair starts at xb = min(x0, W - 2): at the last column x1 == x0 and both taps are its second element
                const int xb = min(x0, p.W - 2);
                const bool first = xb == x0;
                const f32x2_any a0 = *reinterpret_cast<const f32x2_any*>(p.prev + r0 + xb);
                const f32x2_any a1 = *reinterpret_cast<const f32x2_any*>(p.prev + r1 + xb);
                const unsigned b0 = *reinterpret_cast<const u16_any*>(p.grey_prev + r0 + xb);
                const unsigned b1 = *reinterpret_cast<const u16_any*>(p.grey_prev + r1 + xb);
                v00 = first ? a0.x : a0.y, v01 = a0.y, v10 = first ? a1.x : a1.y, v11 = a1.y;
                g01 = (float)(b0 >> 8), g11 = (float)(b1 >> 8);
                g00 = first ? (float)(b0 & 255u) : g01, g10 = first ? (float)(b1 & 255u) : g11;
            } else {
                v00 = v01 = p.prev[r0 + x0], v10 = v11 = p.prev[r1 + x0];
                g00 = g01 = (float)p.grey_prev[r0 + x0], g10 = g11 = (float)p.grey_prev[r1 + x0];
            }
            {
                const float top = (ofx * v00) + (fx * v01), bot = (ofx * v10) + (fx * v11);
                sw = (ofy * top) + (fy * bot);
            }
            float gw;
            {
                const float top = (ofx * g00) + (fx * g01), bot = (ofx * g10) + (fx * g11);
                gw = (ofy * top) + (fy * bot);
            }
            const float wc = ramp0(1.f - fabsf((float)g - gw) * p.inv_tau_colour);      // photometric residual = occlusion test
            const float wa = ramp0(1.f - fabsf(a - sw) * p.inv_tau_alpha);              // a real change of alpha stays
            w = ((p.strength * wc) * wa) * gate;
        }
    }
    const float o = a + (w * (sw - a));
    return finite_f(a) ? clamp01(o) : a;
}

// (uint8) trunc(out * 255) of the clamped value: the byte otvm_crop_outputs writes; a non-finite alpha gives 0
__device__ __forceinline__ unsigned byte_of(float out) { return finite_f(out) ? (unsigned)(int)truncf(out * 255.f) : 0u; }

// vec: rows of whole 16-byte groups (W % 4 == 0, aligned bases); vec_tri: the trimap is at the frame's own resolution and
// aligned, so a group's three classes come as three 16-byte loads
__global__ __launch_bounds__(256) void temporal_blend_kernel(const otvm_temporal_params p, const int vec, const int vec_tri) {
    const int n4 = (p.W + 3) >> 2;
    const int64_t total = (int64_t)p.H * n4;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = p.W - x0 < 4 ? p.W - x0 : 4;
        const int64_t o = (int64_t)y * p.W + x0;
        const bool full = n == 4 && vec;
        const bool moving = p.prev != nullptr, gated = moving && p.tri != nullptr;
        float a[4], dx[4] = {0.f, 0.f, 0.f, 0.f}, dy[4] = {0.f, 0.f, 0.f, 0.f};
        float gate[4] = {1.f, 1.f, 1.f, 1.f};
        unsigned g[4] = {0u, 0u, 0u, 0u};
        if (full) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(p.alpha + o);
            a[0] = av.x, a[1] = av.y, a[2] = av.z, a[3] = av.w;
            if (moving) {
                const f32x4 f0 = *reinterpret_cast<const f32x4*>(p.flow + o * 2);
                const f32x4 f1 = *reinterpret_cast<const f32x4*>(p.flow + o * 2 + 4);
                dx[0] = f0.x, dy[0] = f0.y, dx[1] = f0.z, dy[1] = f0.w, dx[2] = f1.x, dy[2] = f1.y, dx[3] = f1.z, dy[3] = f1.w;
                const unsigned gv = *reinterpret_cast<const unsigned*>(p.grey + o);
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k] = (gv >> (8 * k)) & 255u;
            }
            if (gated && vec_tri) {
                const int64_t plane = (int64_t)p.H * p.W;
                const f32x4 t0 = *reinterpret_cast<const f32x4*>(p.tri + o);
                const f32x4 t1 = *reinterpret_cast<const f32x4*>(p.tri + plane + o);
                const f32x4 t2 = *reinterpret_cast<const f32x4*>(p.tri + 2 * plane + o);
                gate[0] = gate_of(t0.x, t1.x, t2.x), gate[1] = gate_of(t0.y, t1.y, t2.y);
                gate[2] = gate_of(t0.z, t1.z, t2.z), gate[3] = gate_of(t0.w, t1.w, t2.w);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < n;
                a[k] = in ? p.alpha[o + k] : 0.f;
                if (in && moving) {
                    dx[k] = p.flow[(o + k) * 2], dy[k] = p.flow[(o + k) * 2 + 1];
                    g[k] = p.grey[o + k];
                }
            }
        }
        if (gated && !(full && vec_tri)) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) gate[k] = gate_at(p, x0 + k, y);
        }
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = k < n ? blend_pixel(p, x0 + k, y, a[k], g[k], dx[k], dy[k], gate[k]) : 0.f;
        if (full) {
            *reinterpret_cast<f32x4*>(p.out + o) = f32x4{r[0], r[1], r[2], r[3]};
            if (p.out_u8)
                *reinterpret_cast<unsigned*>(p.out_u8 + o) = byte_of(r[0]) | (byte_of(r[1]) << 8) | (byte_of(r[2]) << 16) | (byte_of(r[3]) << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    p.out[o + k] = r[k];
                    if (p.out_u8) p.out_u8[o + k] = (uint8_t)byte_of(r[k]);
                }
        }
    }
}

inline unsigned grid_for(int64_t threads) {
    const int64_t b = (threads + 255) / 256;
    return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));       // grid-stride beyond: any H x W is covered
}

}  // namespace

extern "C" int otvm_luma_u8(const uint8_t* img, int H, int W, int u8_rgb, uint8_t* grey, void* stream) {
    OTVM_REQUIRE(img && grey, "otvm_luma_u8: null image / output");
    OTVM_REQUIRE(H >= 1 && H <= 65535 && W >= 1, "otvm_luma_u8: H is 1 ... 65535 and W >= 1, got %d x %d", W, H);
    const int64_t N = (int64_t)H * W;
    const int vec = (((uintptr_t)img | (uintptr_t)grey) & 15) == 0;
    hipLaunchKernelGGL(luma_u8_kernel, dim3(grid_for((N + 15) >> 4)), dim3(256), 0, (hipStream_t)stream, img, N, u8_rgb ? 1 : 0, grey,
                       vec);
    OTVM_CHECK_LAUNCH("otvm_luma_u8");
    return 0;
}

extern "C" int otvm_temporal_blend(const otvm_temporal_params* p, void* stream) {
    OTVM_REQUIRE(p && p->alpha && p->out, "otvm_temporal_blend: null parameters / alpha / out");
    OTVM_REQUIRE(p->H >= 1 && p->H <= 65535 && p->W >= 1, "otvm_temporal_blend: H is 1 ... 65535 and W >= 1, got %d x %d", p->W, p->H);
    OTVM_REQUIRE(!p->prev || (p->grey && p->grey_prev && p->flow),
                 "otvm_temporal_blend: with a previous alpha the two grey planes and the flow are needed");
    const int64_t N = (int64_t)p->H * p->W;
    OTVM_REQUIRE(!p->prev || p->out + N <= p->prev || p->prev + N <= p->out, "otvm_temporal_blend: out must not alias prev");
    OTVM_REQUIRE(!p->tri || (p->th >= 1 && p->tw >= 1 && p->tri_scale >= 1),
                 "otvm_temporal_blend: a trimap needs th, tw, tri_scale >= 1, got %d x %d at scale %d", p->tw, p->th, p->tri_scale);
    OTVM_REQUIRE(p->strength >= 0.f && p->strength <= 1.f, "otvm_temporal_blend: strength lies in [0,1], got %g", (double)p->strength);
    OTVM_REQUIRE(p->inv_tau_colour > 0.f && p->inv_tau_colour < __builtin_inff() && p->inv_tau_alpha > 0.f &&
                     p->inv_tau_alpha < __builtin_inff(),
                 "otvm_temporal_blend: the reciprocal taus are positive and finite, got %g and %g", (double)p->inv_tau_colour,
                 (double)p->inv_tau_alpha);
    OTVM_REQUIRE((((uintptr_t)p->alpha | (uintptr_t)p->prev | (uintptr_t)p->flow | (uintptr_t)p->tri | (uintptr_t)p->out) & 3) == 0,
                 "otvm_temporal_blend: alpha / prev / flow / tri / out must be 4-byte aligned");
    const int vec = (p->W & 3) == 0 && (((uintptr_t)p->alpha | (uintptr_t)p->flow | (uintptr_t)p->out) & 15) == 0 &&
                    (((uintptr_t)p->grey | (uintptr_t)p->out_u8) & 3) == 0;
    const int vec_tri = p->tri && p->tri_scale == 1 && p->th == p->H && p->tw == p->W && ((uintptr_t)p->tri & 15) == 0;
    hipLaunchKernelGGL(temporal_blend_kernel, dim3(grid_for((int64_t)p->H * ((p->W + 3) / 4))), dim3(256), 0, (hipStream_t)stream, *p,
                       vec, vec_tri);
    OTVM_CHECK_LAUNCH("otvm_temporal_blend");
    return 0;
}
