// Trimap from a segmentation mask (include/otvm_hip.h: otvm_trimap_from_mask): exact erosion of the thresholded mask by
// Euclidean discs, in integer arithmetic.
//   FG = (m >= hi), BG = (m <= lo);  fg = FG and d_FG > t_fg,  bg = BG and d_BG > t_bg,  unknown elsewhere, with d_S(p) the
//   squared distance from p to the nearest in-image pixel outside S (pixels beyond the image seed nothing).
// Only the comparison with t matters, so nothing farther than R = floor(sqrt(t)) is looked at:
//   pass 1 (columns): a pixel belongs to FG, to BG or to neither, so the vertical distance to the nearest non-member of its
//                     own set is the distance to the nearest pixel of its column with ANOTHER class: one run-length scan down
//                     and one up serve both sets.  Out: uint16 [H,W], class << MT_CLS_SHIFT | min(distance, MT_CAP)
//                     (MT_CAP = 256 > any R: the cap never changes a comparison; a run that reaches the image edge has no
//                     non-member on that side and saturates);
//   pass 2 (rows)   : a workgroup takes MT_TILE pixels of one row, stages their packed values and R more on either side in LDS
//                     as squared distances per set (0 where the pixel is no member: it is its own neighbour's non-member) and
//                     every pixel scans outwards until g^2 + dx^2 <= t or |dx| > R.  It writes the one-hot planes and / or the
//                     label bytes.
// No atomics, no initialised workspace: two calls give equal bits.
//
// Size-selected paths (tests/mask_trimap_cases.py holds one size on each side of every line):
//   columns, rows per thread: H <= 512 -> 8 | 513 .. 1280 -> 20 | 1281 .. 2560 -> 40 (a column is cut into 64 segments, one
//            thread each, the rows of a segment in registers) | H > 2560 -> one thread per column, two serial sweeps;
//   rows, segments         : W <= 1024 -> one workgroup per row | W > 1024 -> ceil(W / 1024) workgroups per row, each with
//            its own halo;
//   rows, stores           : W % 4 == 0 and 16-byte aligned trimap / 4-byte aligned labels -> four pixels per store (float4
//            per plane, uchar4) | otherwise pixel by pixel.
#include "common.h"

namespace {

typedef float mt_f32x4 __attribute__((ext_vector_type(4)));
constexpr int MT_CAP = 256;              // > floor(sqrt(65025)) = 255
constexpr int MT_CLS_SHIFT = 12;         // packed: class (0 bg, 1 neither, 2 fg) << 12 | capped distance (1 .. 256)
constexpr int MT_SEGS = 64, MT_XB = 16;  // column pass: segments per column, columns per workgroup
constexpr int MT_TILE = 1024, MT_RMAX = 255;
constexpr int MT_FAR = 1 << 28;          // "no pixel here" (beyond the image): never <= t, and + dx^2 does not overflow

__device__ __forceinline__ int mt_class(int m, int lo, int hi) { return m >= hi ? 2 : (m <= lo ? 0 : 1); }
__device__ __forceinline__ int mt_inc(int d) { return d + 1 > MT_CAP ? MT_CAP : d + 1; }

// pass 1.  Workgroup = MT_XB columns x MT_SEGS segments, lanes along x.  A thread loads all rows of its segment first (LEN_MAX
// independent byte loads in flight), publishes the class and the length of the run at the top and at the bottom of its
// segment, takes the run that continues above / below from the other segments' entries, and scans in registers.
template <int LEN_MAX>
__global__ __launch_bounds__(MT_XB * MT_SEGS) void mt_columns_kernel(const uint8_t* __restrict__ mask, int H, int W, int len, int lo,
                                                                     int hi, uint16_t* __restrict__ g) {
    // per segment and column: rows inside the image | class and run length at the top | class and run length at the bottom
    __shared__ int n_s[MT_SEGS][MT_XB], tcls_s[MT_SEGS][MT_XB], trun_s[MT_SEGS][MT_XB], bcls_s[MT_SEGS][MT_XB], brun_s[MT_SEGS][MT_XB];
    const int lx = threadIdx.x % MT_XB, seg = threadIdx.x / MT_XB;
    const int x = blockIdx.x * MT_XB + lx;
    const int y0 = seg * len;
    const bool live = x < W;
    int n = H - y0 < len ? H - y0 : len;                   // rows of this segment inside the image (<= 0: below it)
    if (n < 0 || !live) n = 0;
    int c[LEN_MAX];
#pragma unroll
    for (int j = 0; j < LEN_MAX; ++j) c[j] = j < n ? mt_class(mask[(int64_t)(y0 + j) * W + x], lo, hi) : -1;
    int trun = 0, brun = 0, bcls = -1;
    {
        bool open = true;
#pragma unroll
        for (int j = 0; j < LEN_MAX; ++j) {
            if (j < n) {
                open = open && c[j] == c[0];
                trun += open ? 1 : 0;
                brun = c[j] == bcls ? brun + 1 : 1;
                bcls = c[j];
            }
        }
    }
    n_s[seg][lx] = n;
    tcls_s[seg][lx] = c[0]; trun_s[seg][lx] = trun;
    bcls_s[seg][lx] = bcls; brun_s[seg][lx] = brun;
    __syncthreads();
    if (n == 0) return;
    // rows directly above the segment that continue the class of its first row; -1: that run reaches the top of the image
    int above = 0;
    {
        int s = seg - 1;
        for (; s >= 0 && above < MT_CAP; --s) {
            if (bcls_s[s][lx] != c[0]) break;
            above += brun_s[s][lx];
            if (brun_s[s][lx] < n_s[s][lx]) break;
        }
        if (s < 0) above = -1;
    }
    int below = 0;
    {
        int s = seg + 1;
        for (; s < MT_SEGS && below < MT_CAP; ++s) {
            if (n_s[s][lx] == 0) { s = MT_SEGS; break; }    // the image ends here
            if (tcls_s[s][lx] != bcls) break;
            below += trun_s[s][lx];
            if (trun_s[s][lx] < n_s[s][lx]) break;
        }
        if (s >= MT_SEGS) below = -1;
    }
    int dn[LEN_MAX];
    int d = above < 0 ? MT_CAP : (above > MT_CAP ? MT_CAP : above);      // row y0 is `above` + 1 rows from the nearest other class over it
#pragma unroll
    for (int j = 0; j < LEN_MAX; ++j) {
        d = (j > 0 && c[j] != c[j - 1]) ? 1 : mt_inc(d);
        dn[j] = d;
    }
    d = below < 0 ? MT_CAP : (below > MT_CAP ? MT_CAP : below);
    uint16_t* gx = g + x;
#pragma unroll
    for (int j = LEN_MAX - 1; j >= 0; --j) {
        if (j < n) {
            d = (j + 1 < n && c[j] != c[j + 1]) ? 1 : mt_inc(d);
            const int v = dn[j] < d ? dn[j] : d;
            gx[(int64_t)(y0 + j) * W] = (uint16_t)((c[j] << MT_CLS_SHIFT) | v);
        }
    }
}

// columns taller than MT_SEGS * 40 rows: one thread per column, a sweep down and a sweep up (slow, rarely used)
__global__ __launch_bounds__(64) void mt_columns_tall_kernel(const uint8_t* __restrict__ mask, int H, int W, int lo, int hi,
                                                             uint16_t* __restrict__ g) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= W) return;
    uint16_t* gx = g + x;
    int d = MT_CAP, prev = -1;
    for (int y = 0; y < H; ++y) {
        const int c = mt_class(mask[(int64_t)y * W + x], lo, hi);
        d = (y > 0 && c != prev) ? 1 : mt_inc(d);
        prev = c;
        gx[(int64_t)y * W] = (uint16_t)((c << MT_CLS_SHIFT) | d);
    }
    d = MT_CAP;
    for (int y = H - 1; y >= 0; --y) {
        const int v = gx[(int64_t)y * W];
        const int c = v >> MT_CLS_SHIFT, dv = v & ((1 << MT_CLS_SHIFT) - 1);
        d = (y < H - 1 && c != prev) ? 1 : mt_inc(d);
        prev = c;
        gx[(int64_t)y * W] = (uint16_t)((c << MT_CLS_SHIFT) | (dv < d ? dv : d));
    }
}

// class of the output at tile position i (pixel of class c, 0 or 2): the pixel keeps its class when no non-member of its set
// lies within squared distance t.  q: the set's squared column distances, tile position 0 at q[0], valid from -R to MT_TILE - 1 + R.
__device__ __forceinline__ int mt_decide(const int* __restrict__ q, int i, int c, int R, int t) {
    if (q[i] <= t) return 1;
    for (int dx = 1; dx <= R; ++dx) {
        const int a = q[i - dx], b = q[i + dx];
        if ((a < b ? a : b) + dx * dx <= t) return 1;
    }
    return c;
}

// pass 2.  grid = (segments of MT_TILE pixels, rows); 256 threads, four consecutive pixels each.
template <bool VEC>
__global__ __launch_bounds__(256) void mt_rows_kernel(const uint16_t* __restrict__ g, int H, int W, int t_fg, int t_bg, int r_fg,
                                                      int r_bg, float* __restrict__ trimap, uint8_t* __restrict__ labels,
                                                      int band_label) {
    __shared__ int q_s[2][MT_TILE + 2 * MT_RMAX];          // [0] the BG set, [1] the FG set
    const int y = blockIdx.y, x0 = blockIdx.x * MT_TILE;
    const int R = r_fg > r_bg ? r_fg : r_bg;
    const int tile = W - x0 < MT_TILE ? W - x0 : MT_TILE;
    const uint16_t* gr = g + (int64_t)y * W;
    for (int i = threadIdx.x; i < tile + 2 * R; i += blockDim.x) {
        const int x = x0 - R + i;
        int qb = MT_FAR, qf = MT_FAR;
        if (x >= 0 && x < W) {
            const int v = gr[x];
            const int c = v >> MT_CLS_SHIFT, d = v & ((1 << MT_CLS_SHIFT) - 1);
            qb = c == 0 ? d * d : 0;
            qf = c == 2 ? d * d : 0;
        }
        q_s[0][i + MT_RMAX - R] = qb;
        q_s[1][i + MT_RMAX - R] = qf;
    }
    __syncthreads();
    const int i0 = threadIdx.x * 4;
    if (i0 >= tile) return;
    int res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = i0 + j;
        res[j] = 1;
        if (i < tile) {
            const int qb = q_s[0][i + MT_RMAX], qf = q_s[1][i + MT_RMAX];
            if (qf > 0) res[j] = mt_decide(q_s[1] + MT_RMAX, i, 2, r_fg, t_fg);
            else if (qb > 0) res[j] = mt_decide(q_s[0] + MT_RMAX, i, 0, r_bg, t_bg);
        }
    }
    const int64_t P = (int64_t)H * W, at = (int64_t)y * W + x0 + i0;
    if (VEC) {                                             // W % 4 == 0: the four pixels lie inside the row
        if (trimap) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                *reinterpret_cast<mt_f32x4*>(trimap + k * P + at) =
                    mt_f32x4{res[0] == k ? 1.f : 0.f, res[1] == k ? 1.f : 0.f, res[2] == k ? 1.f : 0.f, res[3] == k ? 1.f : 0.f};
        }
        if (labels) {
            uchar4 l;
            l.x = (uint8_t)(res[0] == 1 ? band_label : res[0]); l.y = (uint8_t)(res[1] == 1 ? band_label : res[1]);
            l.z = (uint8_t)(res[2] == 1 ? band_label : res[2]); l.w = (uint8_t)(res[3] == 1 ? band_label : res[3]);
            *reinterpret_cast<uchar4*>(labels + at) = l;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < tile) {
                if (trimap) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) trimap[k * P + at + j] = res[j] == k ? 1.f : 0.f;
                }
                if (labels) labels[at + j] = (uint8_t)(res[j] == 1 ? band_label : res[j]);
            }
        }
    }
}

int mt_isqrt(int t) {                                      // floor(sqrt(t)), 0 <= t <= 65025
    int r = 0;
    while ((r + 1) * (r + 1) <= t) ++r;
    return r;
}

}  // namespace

extern "C" int64_t otvm_trimap_from_mask_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || H >= 16384 || W >= 16384) return -1;
    return (int64_t)H * W * 2;
}

extern "C" int otvm_trimap_from_mask(const otvm_mask_trimap_params* p, void* ws, void* stream) {
    OTVM_REQUIRE(p && p->mask && ws, "otvm_trimap_from_mask: null pointer (params, mask or workspace)");
    OTVM_REQUIRE(p->trimap || p->labels, "otvm_trimap_from_mask: neither a trimap nor a label output");
    OTVM_REQUIRE(p->H >= 1 && p->W >= 1 && p->H < 16384 && p->W < 16384, "otvm_trimap_from_mask: the mask is 1 .. 16383 pixels a side, got %dx%d",
                 p->H, p->W);
    OTVM_REQUIRE(0 <= p->lo && p->lo < p->hi && p->hi <= 255, "otvm_trimap_from_mask: thresholds need 0 <= lo < hi <= 255, got %d, %d",
                 p->lo, p->hi);
    OTVM_REQUIRE(p->t_fg >= 0 && p->t_fg <= 65025 && p->t_bg >= 0 && p->t_bg <= 65025,
                 "otvm_trimap_from_mask: squared band widths are 0 .. 65025, got %d, %d", p->t_fg, p->t_bg);
    OTVM_REQUIRE(p->band_label == 1 || p->band_label == 255, "otvm_trimap_from_mask: band_label is 1 (unknown) or 255 (unlabelled), got %d",
                 p->band_label);
    OTVM_REQUIRE(((uintptr_t)ws & 1) == 0 && ((uintptr_t)p->trimap & 3) == 0, "otvm_trimap_from_mask: misaligned workspace or trimap");
    hipStream_t s = (hipStream_t)stream;
    const int H = p->H, W = p->W;
    uint16_t* g = (uint16_t*)ws;
    const int len = otvm_ceil_div(H, MT_SEGS);
    const dim3 cgrid(otvm_ceil_div(W, MT_XB)), cblock(MT_XB * MT_SEGS);
    if (len <= 8) hipLaunchKernelGGL(mt_columns_kernel<8>, cgrid, cblock, 0, s, p->mask, H, W, len, p->lo, p->hi, g);
    else if (len <= 20) hipLaunchKernelGGL(mt_columns_kernel<20>, cgrid, cblock, 0, s, p->mask, H, W, len, p->lo, p->hi, g);
    else if (len <= 40) hipLaunchKernelGGL(mt_columns_kernel<40>, cgrid, cblock, 0, s, p->mask, H, W, len, p->lo, p->hi, g);
    else hipLaunchKernelGGL(mt_columns_tall_kernel, dim3(otvm_ceil_div(W, 64)), dim3(64), 0, s, p->mask, H, W, p->lo, p->hi, g);
    const int r_fg = mt_isqrt(p->t_fg), r_bg = mt_isqrt(p->t_bg);
    const dim3 rgrid(otvm_ceil_div(W, MT_TILE), H);
    const bool vec = W % 4 == 0 && ((uintptr_t)p->trimap & 15) == 0 && ((uintptr_t)p->labels & 3) == 0;
    if (vec) hipLaunchKernelGGL(mt_rows_kernel<true>, rgrid, dim3(256), 0, s, g, H, W, p->t_fg, p->t_bg, r_fg, r_bg, p->trimap, p->labels,
                                p->band_label);
    else hipLaunchKernelGGL(mt_rows_kernel<false>, rgrid, dim3(256), 0, s, g, H, W, p->t_fg, p->t_bg, r_fg, r_bg, p->trimap, p->labels,
                            p->band_label);
    OTVM_CHECK_LAUNCH("otvm_trimap_from_mask");
    return 0;
}
