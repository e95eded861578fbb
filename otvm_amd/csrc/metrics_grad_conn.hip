// Grad and Conn matting metrics on device (reference utils/tmp/metric.py:16-46,191-234) for one frame of 8-bit alphas
// against its ground truth, the companions of metrics.hip's SAD / MSE / dtSSD.
//
// Grad: |grad| of pred and target by the 9x9 Gaussian-derivative filter of sigma 1.4 (genGaussKernel: hx[i][j] =
//   gauss(i-4) dgauss(j-4) / L2 norm, hy = hx^T), applied as a true convolution with replicate padding (the reference flips
//   the kernel and cross-correlates on an edge-replicated frame, ImageFilter.pad).  hx is an outer product, so it runs
//   separably: a row pass with both 1-D factors, then a column pass, in fp64 on an LDS tile.  acc[0] += sum
//   (|grad p| - |grad t|)^2 m.
// Conn: thresholds t_k = float32 arange(0, 1.1, 0.1) (k = 0..10, t_10 = 1.0); m_i = (p/255 >= t_i) & (t/255 >= t_i) is
//   (p >= c_i) & (t >= c_i) with integer cutoffs c_i derived on the host in that float32 arithmetic.  For i = 1..10 the
//   largest 4-connected component of m_i is found; every pixel without a level outside it gets level t_{i-1}; what is left
//   gets 1.0.  acc[1] += sum |phi_p - phi_t| m with phi = 1 - d (d >= 0.15), d = x/255 - level, in float32 as the reference.
//   Every term is a multiple of 2^-26 below 2, so the fp64 sum of a frame up to 2^23 pixels is exact in any order.
//
// Connected components: union-find whose root is the component's minimum linear index (every link points to a smaller
// index), which is the tie-break the reference inherits from skimage's raster-order numbering and np.argmax's first
// maximum.  Per threshold, with kernel boundaries as the only global synchronisation:
//   1 local   : 32x32 tile labelled in LDS (atomicMin union); lab[p] = global index of the tile-local root, cnt[root] = its
//               tile-local size, other cnt = 0
//   2 merge   : union across tile edges on the global label array (atomicMin on roots)
//   3 count   : each tile-local root finds its final root, adds its size there and points at it directly
//   4 argmax  : roots (lab[p] == p) reduce (size << 32 | ~root) with a block max, one 64-bit atomicMax per block
//   5 level   : lab[lab[p]] is p's final root; unassigned pixels outside the winner get level i-1
// Then one kernel computes both per-pixel terms over 32x32 tiles, block partials go to the workspace and one workgroup
// sums them in a fixed order: the result does not depend on scheduling.
#include "common.h"
#include <math.h>

namespace {

constexpr int GC_T = 32;                 // tile side (labelling and filter)
constexpr int GC_R = 4;                  // filter half width (hsize of sigma 1.4)
constexpr int GC_L = GC_T + 2 * GC_R;    // filter input tile side
constexpr int GC_LEVELS = 10;            // thresholds t_1 .. t_10
constexpr uint8_t GC_UNSET = GC_LEVELS;  // level map value "no level yet" = "1.0" once all thresholds are done

struct GcTaps { double g[2 * GC_R + 1], dg[2 * GC_R + 1]; };
struct GcLevels { float t[GC_LEVELS + 1]; };

// ---- constants, host side (also exported for the tests: otvm_matting_grad_conn_params)
void gc_params(int* cut, float* lev, GcTaps* taps) {
    for (int k = 0; k <= GC_LEVELS; ++k)
        lev[k] = (float)(0.0 + (double)k * 0.1);          // torch.arange(0, 1.1, 0.1), float32: start + k*step in double
    for (int i = 1; i <= GC_LEVELS; ++i) {
        int c = 256;                                        // x/255.f is monotone in x: the first x that passes
        for (int x = 255; x >= 0; --x)
            if ((float)x / 255.0f >= lev[i]) c = x;
        cut[i - 1] = c;
    }
    // genGaussKernel(1.4): gauss / dgauss sampled at -4..4; the 2-D L2 norm of the outer product is the product of the norms
    const double sigma = 1.4, pi = 3.14159265358979323846;
    double ng = 0, nd = 0;
    for (int k = 0; k <= 2 * GC_R; ++k) {
        const double x = k - GC_R;
        const double g = exp(-x * x / (2 * sigma * sigma)) / (sigma * sqrt(2 * pi));
        taps->g[k] = g;
        taps->dg[k] = -x * g / (sigma * sigma);
        ng += taps->g[k] * taps->g[k];
        nd += taps->dg[k] * taps->dg[k];
    }
    for (int k = 0; k <= 2 * GC_R; ++k) {
        taps->g[k] /= sqrt(ng);
        taps->dg[k] /= sqrt(nd);
    }
}

__device__ __forceinline__ int gc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gc_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int gc_find(const int* lab, int x) {
    int p;
    while ((p = gc_load(lab + x)) != x) x = p;
    return x;
}

// union of the sets of a and b: the larger root is linked below the smaller one; a failed atomicMin means another thread
// lowered that entry first, and the union goes on from the value it found
__device__ void gc_union(int* lab, int a, int b) {
    for (;;) {
        a = gc_find(lab, a);
        b = gc_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int old = atomicMin(lab + b, a);
            if (old == b) return;
            b = old;
        } else {
            const int old = atomicMin(lab + a, b);
            if (old == a) return;
            a = old;
        }
    }
}

__device__ __forceinline__ int gc_find_lds(const volatile int* L, int x) {
    int p;
    while ((p = L[x]) != x) x = p;
    return x;
}

__device__ void gc_union_lds(int* L, int a, int b) {
    for (;;) {
        a = gc_find_lds(L, a);
        b = gc_find_lds(L, b);
        if (a == b) return;
        if (a < b) {
            const int old = atomicMin(L + b, a);
            if (old == b) return;
            b = old;
        } else {
            const int old = atomicMin(L + a, b);
            if (old == a) return;
            a = old;
        }
    }
}

// phase 1: block (32, 8) labels one 32x32 tile, 4 rows per thread.  Tile-local index ly*32+lx orders the pixels as their
// global indices do, so the local minimum is the global minimum of the tile-local component.
__global__ __launch_bounds__(256) void gc_local_kernel(const uint8_t* __restrict__ p, const uint8_t* __restrict__ t, int H, int W,
                                                       int cut, int level_i, int* __restrict__ lab, unsigned* __restrict__ cnt,
                                                       uint8_t* __restrict__ lev, unsigned long long* __restrict__ best) {
    __shared__ int L[GC_T * GC_T];
    __shared__ unsigned S[GC_T * GC_T];
    const int lx = threadIdx.x, x = blockIdx.x * GC_T + lx, y0 = blockIdx.y * GC_T;
    bool fg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = threadIdx.y + 8 * k, y = y0 + ly, l = ly * GC_T + lx;
        bool f = false;
        if (x < W && y < H) {
            const int64_t g = (int64_t)y * W + x;
            f = p[g] >= cut && t[g] >= cut;
        }
        fg[k] = f;
        L[l] = f ? l : -1;
        S[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = threadIdx.y + 8 * k, l = ly * GC_T + lx;
        if (!fg[k]) continue;
        if (lx > 0 && L[l - 1] >= 0) gc_union_lds(L, l, l - 1);
        if (ly > 0 && L[l - GC_T] >= 0) gc_union_lds(L, l, l - GC_T);
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = (threadIdx.y + 8 * k) * GC_T + lx;
        root[k] = fg[k] ? gc_find_lds(L, l) : -1;
        if (fg[k]) atomicAdd(S + root[k], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = threadIdx.y + 8 * k, y = y0 + ly, l = ly * GC_T + lx;
        if (x >= W || y >= H) continue;
        const int64_t g = (int64_t)y * W + x;
        const int r = root[k];
        lab[g] = r < 0 ? -1 : (int)((int64_t)(y0 + r / GC_T) * W + blockIdx.x * GC_T + r % GC_T);
        cnt[g] = (r >= 0 && r == l) ? S[l] : 0u;
        if (level_i == 1) lev[g] = GC_UNSET;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) *best = 0ull;
}

// phase 2: one 64-thread block per tile: lanes 0-31 join the tile's top row to the row above, lanes 32-63 its left column to
// the column on its left
__global__ __launch_bounds__(64) void gc_merge_kernel(int H, int W, int* __restrict__ lab) {
    const int x0 = blockIdx.x * GC_T, y0 = blockIdx.y * GC_T, j = threadIdx.x & 31;
    int a = -1, b = -1;
    if (threadIdx.x < 32) {
        const int x = x0 + j;
        if (y0 > 0 && x < W) { a = (int)((int64_t)y0 * W + x); b = a - W; }
    } else {
        const int y = y0 + j;
        if (x0 > 0 && y < H) { a = (int)((int64_t)y * W + x0); b = a - 1; }
    }
    if (a >= 0 && gc_load(lab + a) >= 0 && gc_load(lab + b) >= 0) gc_union(lab, a, b);
}

// phase 3: tile-local roots (cnt > 0: only final roots ever receive adds, and they are tile-local roots themselves) move
// their size to the final root and point at it
__global__ __launch_bounds__(256) void gc_count_kernel(int64_t N, int* __restrict__ lab, unsigned* __restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned c = cnt[i];
        if (c == 0) continue;
        const int r = gc_find(lab, (int)i);
        if (r != (int)i) {
            atomicAdd(cnt + r, c);
            gc_store(lab + i, r);
        }
    }
}

// phase 4: the largest component, ties to the smallest root: max of (size << 32 | 0xFFFFFFFF - root)
__global__ __launch_bounds__(256) void gc_argmax_kernel(int64_t N, const int* __restrict__ lab, const unsigned* __restrict__ cnt,
                                                        unsigned long long* __restrict__ best) {
    __shared__ unsigned long long bm;
    if (threadIdx.x == 0) bm = 0ull;
    __syncthreads();
    unsigned long long m = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (lab[i] == (int)i) {
            const unsigned long long k = ((unsigned long long)cnt[i] << 32) | (0xFFFFFFFFull - (unsigned long long)i);
            m = k > m ? k : m;
        }
    }
    if (m) atomicMax(&bm, m);
    __syncthreads();
    if (threadIdx.x == 0 && bm) atomicMax(best, bm);
}

// phase 5: level i-1 for every pixel without a level outside the winning component (an empty m_i has no winner)
__global__ __launch_bounds__(256) void gc_level_kernel(int64_t N, const int* __restrict__ lab, const unsigned long long* __restrict__ best,
                                                       int level_i, uint8_t* __restrict__ lev) {
    const unsigned long long b = *best;
    const int win = (b >> 32) ? (int)(0xFFFFFFFFull - (b & 0xFFFFFFFFull)) : -1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (lev[i] != GC_UNSET) continue;
        const int l = lab[i];
        const bool in = l >= 0 && lab[l] == win;
        if (!in) lev[i] = (uint8_t)(level_i - 1);
    }
}

__device__ __forceinline__ float gc_phi(int x, float level) {
    const float d = (float)x / 255.0f - level;
    return 1.0f - (d >= 0.15f ? d : 0.0f);
}

// per-pixel Grad and Conn terms of a 32x32 tile (block (32, 8), 4 rows per thread); block partials to part[block][2]
__global__ __launch_bounds__(256) void gc_terms_kernel(const uint8_t* __restrict__ p, const uint8_t* __restrict__ t,
                                                       const uint8_t* __restrict__ m, int H, int W, const uint8_t* __restrict__ lev,
                                                       GcTaps taps, GcLevels levels, double* __restrict__ part) {
    __shared__ uint8_t sp[GC_L][GC_L], st[GC_L][GC_L];
    __shared__ double hgp[GC_L][GC_T], hdp[GC_L][GC_T], hgt[GC_L][GC_T], hdt[GC_L][GC_T];
    __shared__ double red[2][256];
    __shared__ float slev[GC_LEVELS + 1];
    const int x0 = blockIdx.x * GC_T, y0 = blockIdx.y * GC_T;
    const int tid = threadIdx.y * GC_T + threadIdx.x;
    if (tid <= GC_LEVELS) slev[tid] = levels.t[tid];
    for (int e = tid; e < GC_L * GC_L; e += 256) {           // replicate padding = clamped coordinates
        const int ry = e / GC_L, rx = e % GC_L;
        const int y = min(max(y0 + ry - GC_R, 0), H - 1), x = min(max(x0 + rx - GC_R, 0), W - 1);
        const int64_t g = (int64_t)y * W + x;
        sp[ry][rx] = p[g];
        st[ry][rx] = t[g];
    }
    __syncthreads();
    // row pass: h[r][c] = sum_v f[4+v] x[r][c-v]  (convolution)
    for (int e = tid; e < GC_L * GC_T; e += 256) {
        const int r = e / GC_T, c = e % GC_T;
        double gp = 0, dp = 0, gt = 0, dt = 0;
#pragma unroll
        for (int k = 0; k <= 2 * GC_R; ++k) {                 // k = 4 + v reads column c + 4 - v = c + 8 - k of the tile
            const double vp = sp[r][c + 2 * GC_R - k] / 255.0, vt = st[r][c + 2 * GC_R - k] / 255.0;
            gp += taps.g[k] * vp; dp += taps.dg[k] * vp;
            gt += taps.g[k] * vt; dt += taps.dg[k] * vt;
        }
        hgp[r][c] = gp; hdp[r][c] = dp; hgt[r][c] = gt; hdt[r][c] = dt;
    }
    __syncthreads();
    double sg = 0, sc = 0;
    const int c = threadIdx.x, x = x0 + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = threadIdx.y + 8 * q, y = y0 + r;
        if (x >= W || y >= H) continue;
        // gx = sum_u g[4+u] (row pass with dg)[r-u];  gy = sum_u dg[4+u] (row pass with g)[r-u]
        double gxp = 0, gyp = 0, gxt = 0, gyt = 0;
#pragma unroll
        for (int k = 0; k <= 2 * GC_R; ++k) {
            const int rr = r + 2 * GC_R - k;
            gxp += taps.g[k] * hdp[rr][c]; gyp += taps.dg[k] * hgp[rr][c];
            gxt += taps.g[k] * hdt[rr][c]; gyt += taps.dg[k] * hgt[rr][c];
        }
        const int64_t g = (int64_t)y * W + x;
        if (m && m[g] == 0) continue;
        const double e = sqrt(gxp * gxp + gyp * gyp) - sqrt(gxt * gxt + gyt * gyt);
        sg += e * e;
        const float level = slev[lev[g]];
        sc += (double)fabsf(gc_phi(sp[r + GC_R][c + GC_R], level) - gc_phi(st[r + GC_R][c + GC_R], level));
    }
    red[0][tid] = sg;
    red[1][tid] = sc;
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

// fixed-order sum of the block partials into acc[0..1]
__global__ __launch_bounds__(256) void gc_finish_kernel(const double* __restrict__ part, int nb, double* __restrict__ acc) {
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

inline int64_t gc_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct GcWs { int* lab; unsigned* cnt; uint8_t* lev; unsigned long long* best; double* part; int64_t bytes; };

GcWs gc_ws_layout(int H, int W, void* base) {
    const int64_t N = (int64_t)H * W, nb = (int64_t)otvm_ceil_div(W, GC_T) * otvm_ceil_div(H, GC_T);
    const uintptr_t b = (uintptr_t)base;
    GcWs w;
    int64_t o = 0;
    w.lab = (int*)(b + o); o += gc_align(4 * N);
    w.cnt = (unsigned*)(b + o); o += gc_align(4 * N);
    w.lev = (uint8_t*)(b + o); o += gc_align(N);
    w.best = (unsigned long long*)(b + o); o += gc_align(8);
    w.part = (double*)(b + o); o += gc_align(16 * nb);
    w.bytes = o;
    return w;
}

}  // namespace

extern "C" int otvm_matting_grad_conn_params(int* cutoffs, float* levels, double* taps) {
    int cut[GC_LEVELS];
    float lev[GC_LEVELS + 1];
    GcTaps tp;
    gc_params(cut, lev, &tp);
    if (cutoffs) for (int i = 0; i < GC_LEVELS; ++i) cutoffs[i] = cut[i];
    if (levels) for (int i = 0; i <= GC_LEVELS; ++i) levels[i] = lev[i];
    if (taps) for (int i = 0; i <= 2 * GC_R; ++i) { taps[i] = tp.g[i]; taps[2 * GC_R + 1 + i] = tp.dg[i]; }
    return 0;
}

extern "C" int64_t otvm_matting_grad_conn_ws_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return gc_ws_layout(H, W, nullptr).bytes;
}

extern "C" int otvm_matting_grad_conn(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, int H, int W, double* acc,
                                      uint8_t* level_map, void* ws, void* stream) {
    OTVM_REQUIRE(pred && target && acc && ws && H > 0 && W > 0, "otvm_matting_grad_conn: bad arguments");
    const int64_t N = (int64_t)H * W;
    OTVM_REQUIRE(N < ((int64_t)1 << 31) - 1, "otvm_matting_grad_conn: %d x %d pixels exceed 32-bit labels", H, W);
    static int cut[GC_LEVELS];
    static GcLevels levels;
    static GcTaps taps;
    static const bool init = (gc_params(cut, levels.t, &taps), true);
    (void)init;
    hipStream_t s = (hipStream_t)stream;
    GcWs w = gc_ws_layout(H, W, ws);
    uint8_t* lev = level_map ? level_map : w.lev;
    const dim3 tiles(otvm_ceil_div(W, GC_T), otvm_ceil_div(H, GC_T));
    const int nb = (int)(tiles.x * tiles.y);
    const int64_t nflat = (N + 255) / 256;
    const int gflat = (int)(nflat > 2048 ? 2048 : nflat);
    for (int i = 1; i <= GC_LEVELS; ++i) {
        hipLaunchKernelGGL(gc_local_kernel, tiles, dim3(GC_T, 8), 0, s, pred, target, H, W, cut[i - 1], i, w.lab, w.cnt, lev, w.best);
        hipLaunchKernelGGL(gc_merge_kernel, tiles, dim3(64), 0, s, H, W, w.lab);
        hipLaunchKernelGGL(gc_count_kernel, dim3(gflat), dim3(256), 0, s, N, w.lab, w.cnt);
        hipLaunchKernelGGL(gc_argmax_kernel, dim3(gflat), dim3(256), 0, s, N, (const int*)w.lab, (const unsigned*)w.cnt, w.best);
        hipLaunchKernelGGL(gc_level_kernel, dim3(gflat), dim3(256), 0, s, N, (const int*)w.lab, (const unsigned long long*)w.best, i, lev);
        OTVM_CHECK_LAUNCH("otvm_matting_grad_conn (components)");
    }
    hipLaunchKernelGGL(gc_terms_kernel, tiles, dim3(GC_T, 8), 0, s, pred, target, mask, H, W, (const uint8_t*)lev, taps, levels, w.part);
    hipLaunchKernelGGL(gc_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)w.part, nb, acc);
    OTVM_CHECK_LAUNCH("otvm_matting_grad_conn");
    return 0;
}
