// Masks of keyed footage (include/otvm_hip.h: otvm_mask_from_chroma, otvm_mask_from_plate): the frame itself -> the uint8 [H,W]
// mask otvm_trimap_from_mask takes (255 subject, 0 screen / plate).  Integer arithmetic only (the header states every operation;
// tests/key_ref.py restates both kernels and is compared bit for bit), no atomics, every element of the mask written.
//
// Both are 8 MB passes at 1920x1080 (6.2 MB of frame in, 2.1 MB of mask out; the plate key reads the plate as well).  A thread
// takes four consecutive pixels of one output row: when W % 4 == 0 and the bases are dword-aligned (VEC) the twelve colour bytes
// move as three dwords and the four mask bytes as one, otherwise pixel by pixel -- the pattern of window_ops.h.  Offsets are 64-bit.
//
// The chroma key is a pure streaming pass, grid-stride, no LDS.  The plate key is a (2r+1)^2 stencil over the PLATE: a workgroup of
// 256 threads owns a tile of 16 rows x 64 columns (16 threads x 4 pixels across), stages the plate tile with its halo -- coordinates
// clamped to the image -- in LDS as one dword per pixel, and reads the frame once from global memory.  A thread's window of
// 4 + 2r <= 10 pixels starts at dword 4 * tx, 16-byte aligned, so it is read as one to three 16-byte quads per LDS row
// (ds_read_b128).  The LDS row pitch is 128 dwords, a multiple of the 64 banks: the 16-lane groups that instruction is serviced in
// are NOT the 16 lanes of one tile row -- the first is lanes 0-3, 12-15 (row ty) and 20-27 (row ty + 1) -- and with a pitch of
// 0 mod 64 the pieces of a group from two tile rows fall on complementary banks (0-15, 48-63 and 16-47), so a quad read has no
// conflict; a pitch of 72 would put lanes 12-13 and 26-27 on the same banks (2-way).  (22 x 128 x 4 = 11264 bytes at r = 3.)
#include "common.h"

namespace {

constexpr int KEY_MAX_SIDE = 16383;
constexpr int KEY_MAX_BLOCKS = 2048;
// the chroma rows of BT.601 full range, 20 fractional bits: yuv.hip's kFwd[BT601][FULL] (UG = CH - UR, VG = CH - VB)
constexpr int KEY_CH = 524288, KEY_UR = 176932, KEY_VB = 85262;

constexpr int PT_ROWS = 16, PT_COLS = 64, PT_PITCH = 128;     // the plate key's tile and its LDS row pitch in dwords

__device__ __forceinline__ int key_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool VEC>
__device__ __forceinline__ void key_load4(const uint8_t* __restrict__ q, int n, unsigned (&b)[12]) {
    if (VEC) {
        const unsigned* w = reinterpret_cast<const unsigned*>(q);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const unsigned v = w[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[4 * i + j] = (v >> (8 * j)) & 255u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) b[j] = j < 3 * n ? (unsigned)q[j] : 0u;
    }
}

template <bool VEC>
__device__ __forceinline__ void key_store4(uint8_t* __restrict__ o, int n, const unsigned (&m)[4]) {
    if (VEC) {
        *reinterpret_cast<unsigned*>(o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) o[j] = (uint8_t)m[j];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void mask_from_chroma_kernel(const otvm_mask_from_chroma_params p) {
    const int H = p.H, W = p.W, n4 = (W + 3) >> 2;
    const int kb = p.kb, kr = p.kr, qlo = p.qlo, span = p.qhi - p.qlo;
    const int ri = p.u8_rgb ? 0 : 2, bi = 2 - ri;
    const int64_t total = (int64_t)H * n4;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / n4), x0 = (int)(t - (int64_t)y * n4) * 4;
        const int n = W - x0 < 4 ? W - x0 : 4;
        const int64_t o = (int64_t)y * W + x0;
        unsigned b[12], m[4];
        key_load4<VEC>(p.frame + o * 3, n, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int R = (int)b[3 * j + ri], G = (int)b[3 * j + 1], B = (int)b[3 * j + bi];
            const int bias = (128 << 20) + (1 << 19);
            const int cb = key_clamp((-KEY_UR * R - (KEY_CH - KEY_UR) * G + KEY_CH * B + bias) >> 20, 0, 255) - 128;
            const int cr = key_clamp((KEY_CH * R - (KEY_CH - KEY_VB) * G - KEY_VB * B + bias) >> 20, 0, 255) - 128;
            const int cross = cb * kr - cr * kb;
            const int q = cb * kb + cr * kr - (cross < 0 ? -cross : cross);
            const int d = q - qlo;
            m[j] = d <= 0 ? 255u : (d >= span ? 0u : (unsigned)(255 - (d * 255) / span));
        }
        key_store4<VEC>(p.mask + o, n, m);
    }
}

template <int R, bool VEC>
__global__ __launch_bounds__(256) void mask_from_plate_kernel(const otvm_mask_from_plate_params p, const int tiles_x) {
    constexpr int LR = PT_ROWS + 2 * R, LC = PT_COLS + 2 * R;      // staged rows and columns
    constexpr int NQ = (4 + 2 * R + 3) / 4;                          // 16-byte quads of a thread's window per LDS row
    __shared__ __attribute__((aligned(16))) unsigned plate_s[LR * PT_PITCH];
    const int H = p.H, W = p.W;
    const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
    const int ty0 = tile_y * PT_ROWS, tx0 = tile_x * PT_COLS;
    for (int i = threadIdx.x; i < LR * LC; i += 256) {
        const int ly = i / LC, lx = i - ly * LC;
        const int gy = key_clamp(ty0 - R + ly, 0, H - 1), gx = key_clamp(tx0 - R + lx, 0, W - 1);
        const uint8_t* q = p.plate + ((int64_t)gy * W + gx) * 3;
        plate_s[ly * PT_PITCH + lx] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int y = ty0 + ty, x0 = tx0 + 4 * tx;
    if (y >= H || x0 >= W) return;                                   // (after the only barrier)
    const int n = W - x0 < 4 ? W - x0 : 4;
    const int64_t o = (int64_t)y * W + x0;
    unsigned b[12], m[4];
    key_load4<VEC>(p.frame + o * 3, n, b);
    int d[4] = {255, 255, 255, 255};
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy) {
        unsigned win[4 * NQ];                                        // plate pixels x0 - R ... of row y - R + dy
        const uint4* row = reinterpret_cast<const uint4*>(plate_s + (ty + dy) * PT_PITCH + 4 * tx);
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const uint4 v = row[k];
            win[4 * k] = v.x; win[4 * k + 1] = v.y; win[4 * k + 2] = v.z; win[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c0 = (int)b[3 * j], c1 = (int)b[3 * j + 1], c2 = (int)b[3 * j + 2];
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) {
                const unsigned v = win[j + dx];
                int e0 = c0 - (int)(v & 255u), e1 = c1 - (int)((v >> 8) & 255u), e2 = c2 - (int)((v >> 16) & 255u);
                e0 = e0 < 0 ? -e0 : e0;
                e1 = e1 < 0 ? -e1 : e1;
                e2 = e2 < 0 ? -e2 : e2;
                const int e = e0 > e1 ? (e0 > e2 ? e0 : e2) : (e1 > e2 ? e1 : e2);
                d[j] = e < d[j] ? e : d[j];
            }
        }
    }
    const int lo = p.lo, span = p.hi - p.lo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = d[j] - lo;
        m[j] = v <= 0 ? 0u : (v >= span ? 255u : (unsigned)((v * 255) / span));
    }
    key_store4<VEC>(p.mask + o, n, m);
}

int key_common_ok(const char* name, const void* frame, const void* mask, int H, int W) {
    OTVM_REQUIRE(H >= 1 && H <= KEY_MAX_SIDE && W >= 1 && W <= KEY_MAX_SIDE, "%s: sides are 1 ... 16383, got %d x %d", name, W, H);
    OTVM_REQUIRE(frame && mask, "%s: null frame / mask", name);
    return 0;
}

bool key_vec(int W, const void* a, const void* b) { return (W & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 3) == 0; }

template <int R>
void launch_plate(const otvm_mask_from_plate_params& p, bool vec, unsigned blocks, int tiles_x, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((mask_from_plate_kernel<R, true>), dim3(blocks), dim3(256), 0, s, p, tiles_x);
    else     hipLaunchKernelGGL((mask_from_plate_kernel<R, false>), dim3(blocks), dim3(256), 0, s, p, tiles_x);
}

}  // namespace

extern "C" int otvm_mask_from_chroma(const otvm_mask_from_chroma_params* p, void* stream) {
    const char* name = "otvm_mask_from_chroma";
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (int rc = key_common_ok(name, p->frame, p->mask, p->H, p->W)) return rc;
    OTVM_REQUIRE(p->kb >= -128 && p->kb <= 127 && p->kr >= -128 && p->kr <= 127, "%s: the key's chroma (kb, kr) is -128 ... 127, got %d, %d",
                 name, p->kb, p->kr);
    OTVM_REQUIRE(p->kb * p->kb + p->kr * p->kr >= 256, "%s: the key colour is grey (kb^2 + kr^2 = %d < 16^2): it has no hue to key on", name,
                 p->kb * p->kb + p->kr * p->kr);
    OTVM_REQUIRE(p->qlo >= -(1 << 20) && p->qhi <= (1 << 20), "%s: the thresholds are -2^20 ... 2^20, got qlo=%d qhi=%d", name, p->qlo,
                 p->qhi);
    OTVM_REQUIRE(p->qlo < p->qhi, "%s: the thresholds need qlo < qhi, got qlo=%d qhi=%d", name, p->qlo, p->qhi);
    const int64_t threads = (int64_t)p->H * ((p->W + 3) >> 2);
    const int64_t blocks = (threads + 255) >> 8;
    const dim3 grid((unsigned)(blocks > KEY_MAX_BLOCKS ? KEY_MAX_BLOCKS : blocks));
    if (key_vec(p->W, p->frame, p->mask))
        hipLaunchKernelGGL((mask_from_chroma_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    else
        hipLaunchKernelGGL((mask_from_chroma_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, *p);
    OTVM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int otvm_mask_from_plate(const otvm_mask_from_plate_params* p, void* stream) {
    const char* name = "otvm_mask_from_plate";
    OTVM_REQUIRE(p, "%s: null parameters", name);
    if (int rc = key_common_ok(name, p->frame, p->mask, p->H, p->W)) return rc;
    OTVM_REQUIRE(p->plate, "%s: null plate", name);
    OTVM_REQUIRE(p->radius >= 0 && p->radius <= 3, "%s: radius is 0 ... 3, got %d", name, p->radius);
    OTVM_REQUIRE(0 <= p->lo && p->lo < p->hi && p->hi <= 255, "%s: the thresholds need 0 <= lo < hi <= 255, got lo=%d hi=%d", name, p->lo,
                 p->hi);
    const int tiles_x = (p->W + PT_COLS - 1) / PT_COLS, tiles_y = (p->H + PT_ROWS - 1) / PT_ROWS;
    const unsigned blocks = (unsigned)tiles_x * (unsigned)tiles_y;             // at most 256 x 1024
    const bool vec = key_vec(p->W, p->frame, p->mask);
    hipStream_t s = (hipStream_t)stream;
    switch (p->radius) {
        case 0: launch_plate<0>(*p, vec, blocks, tiles_x, s); break;
        case 1: launch_plate<1>(*p, vec, blocks, tiles_x, s); break;
        case 2: launch_plate<2>(*p, vec, blocks, tiles_x, s); break;
        default: launch_plate<3>(*p, vec, blocks, tiles_x, s); break;
    }
    OTVM_CHECK_LAUNCH(name);
    return 0;
}
