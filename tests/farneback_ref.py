"""CPU restatement of OpenCV 4.x calcOpticalFlowFarneback with the reference's fixed arguments, and of MESSDdt
(reference utils/tmp/metric.py:48-53,266-302).  TEST INFRASTRUCTURE.

calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 10, 2, 7, 1.5, OPTFLOW_FARNEBACK_GAUSSIAN): pyr_scale 0.5, up to 5
pyramid levels (a level must keep both sides >= 32), winsize 10, 2 iterations, poly_n 7, poly_sigma 1.5, Gaussian window.
Neither cv2 nor OpenCV's source is available to the project: this follows OpenCV's optflowgf.cpp / GaussianBlur / resize as
DESIGN.md section 3 states them and is checked against cv2 by definition only.

dtype=np.float32 restates OpenCV's arithmetic: every float32 operation in OpenCV's order, the double accumulations of
FarnebackPolyExp and the double solve.  dtype=np.float64 evaluates the same algorithm with every quantity in float64
(kernel taps included): the precision yardstick of the float32 evaluations.

Operation orders (the device kernels, csrc/optflow_farneback.hip, use the same ones):
  GaussianBlur, row filter first:  ksize 3: x[c]*k_c + (x[c-1] + x[c+1])*k_s;  ksize > 3: k[0]*x[c-r], then += k[j]*x[c-r+j]
               column filter:      ksize 3: (x[r-1] + x[r+1])*k_s + x[r]*k_c;  ksize > 3: k_c*x[r], then += k_i*(x[r+i] + x[r-i])
               border REFLECT_101
  resize INTER_LINEAR: (S[sx]*a0 + S[sx+1]*a1) per source row, then h0*b0 + h1*b1; an exact 2x downscale in both axes is
               OpenCV's area path ((a + b) + (c + d))*0.25
"""
import math

import numpy as np

PYR_SCALE, NUM_LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA = 0.5, 5, 10, 2, 7, 1.5
MIN_SIZE = 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


def cv_round(x):
    """cvRound: round half to even."""
    return int(np.rint(x))


def level_table(H, W):
    """[(k, width, height, ksize, sigma)] for the levels k = L .. 0 in processing order."""
    scale, k = 1.0, 0
    while k < NUM_LEVELS:
        scale *= PYR_SCALE
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    out = []
    for lv in range(k, -1, -1):
        scale = 1.0
        for _ in range(lv):
            scale *= PYR_SCALE
        sigma = (1.0 / scale - 1) * 0.5
        ks = max(cv_round(sigma * 5) | 1, 3)
        out.append((lv, cv_round(W * scale), cv_round(H * scale), ks, sigma))
    return out


def gaussian_kernel(ksize, sigma, dtype=np.float32):
    """getGaussianKernel(ksize, sigma): the fixed [0.25, 0.5, 0.25] for ksize 3 and sigma 0, else exp(-x^2 / (2 sigma^2))
    normalised in double (OpenCV's bit-exact summation order: the half below the centre, doubled, plus the centre)."""
    if sigma <= 0:
        assert ksize == 3
        return np.array([0.25, 0.5, 0.25], dtype)
    n2 = (ksize - 1) // 2
    scale2x = -0.125 / (sigma * sigma)
    vals, s = [], 0.0
    for i in range(n2):
        x = 1 - ksize + 2 * i
        t = math.exp(float(x * x) * scale2x)
        vals.append(t)
        s += t
    s = s * 2.0 + 1.0
    vals.append(1.0)
    half = [v / s for v in vals]
    return np.array(half + half[-2::-1], dtype)


def reflect101(i, n):
    """BORDER_REFLECT_101 index (an axis of length 1 maps everything to 0)."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i
        i = np.where(lo, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)


def resize_coeffs(n_src, n_dst, dtype):
    """INTER_LINEAR source indices and weights along one axis: fx = (d + 0.5) * (n_src / n_dst) - 0.5 (double, stored as
    dtype), sx = floor; below 0 -> (0, fx 0), at or past the last source pixel -> (last, fx 0).  Returns (sx, sx1, 1-fx, fx)."""
    scale = 1.0 / (float(n_dst) / n_src)
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(dtype)
    s = np.floor(f)
    f = (f - s).astype(dtype)
    s = s.astype(np.int64)
    low = s < 0
    s, f = np.where(low, 0, s), np.where(low, dtype(0), f).astype(dtype)
    high = s >= n_src - 1
    s, f = np.where(high, n_src - 1, s), np.where(high, dtype(0), f).astype(dtype)
    return s, np.minimum(s + 1, n_src - 1), (dtype(1) - f).astype(dtype), f


def _row_filter(src, cols, k):
    """Row pass of the separable Gaussian at the source columns `cols`, every row of src."""
    W = src.shape[1]
    r = len(k) // 2
    if len(k) == 3:
        return src[:, cols] * k[1] + (src[:, reflect101(cols - 1, W)] + src[:, reflect101(cols + 1, W)]) * k[0]
    s = k[0] * src[:, reflect101(cols - r, W)]
    for j in range(1, len(k)):
        s = s + k[j] * src[:, reflect101(cols - r + j, W)]
    return s


def _col_filter(hb, rows, k):
    """Column pass at the source rows `rows` of the row-filtered columns hb."""
    H = hb.shape[0]
    r = len(k) // 2
    if len(k) == 3:
        return (hb[reflect101(rows - 1, H)] + hb[reflect101(rows + 1, H)]) * k[0] + hb[rows] * k[1]
    s = k[r] * hb[rows]
    for i in range(1, r + 1):
        s = s + k[r + i] * (hb[reflect101(rows + i, H)] + hb[reflect101(rows - i, H)])
    return s


def level_image(u8, width, height, ksize, sigma, dtype=np.float32):
    """GaussianBlur(full-resolution frame, ksize, sigma, REFLECT_101) resized to width x height (INTER_LINEAR).  Only the
    blurred values the resize reads are computed: bit-identical to blurring the whole frame, then resizing."""
    src = np.asarray(u8).astype(dtype)
    H, W = src.shape
    k = gaussian_kernel(ksize, sigma, dtype)
    if width == W and height == H:                      # resize to the same size is a copy
        return _col_filter(_row_filter(src, np.arange(W), k), np.arange(H), k)
    sx0, sx1, a0, a1 = resize_coeffs(W, width, dtype)
    sy0, sy1, b0, b1 = resize_coeffs(H, height, dtype)
    hb = _row_filter(src, np.stack([sx0, sx1], 1).ravel(), k)          # [H, 2*width]: columns sx0, sx1 of each output
    c0, c1 = _col_filter(hb, sy0, k), _col_filter(hb, sy1, k)         # [height, 2*width]
    a, b, c, d = c0[:, 0::2], c0[:, 1::2], c1[:, 0::2], c1[:, 1::2]
    if W == 2 * width and H == 2 * height:              # OpenCV's area path for an exact 2x downscale
        return ((a + b) + (c + d)) * dtype(0.25)
    h0 = a * a0 + b * a1
    h1 = c * a0 + d * a1
    return h0 * b0[:, None] + h1 * b1[:, None]


def resize_linear(img, width, height, dtype=np.float32):
    """INTER_LINEAR resize of a [h, w, C] array (the flow upscale between levels)."""
    h, w = img.shape[:2]
    sx0, sx1, a0, a1 = resize_coeffs(w, width, dtype)
    sy0, sy1, b0, b1 = resize_coeffs(h, height, dtype)
    a0, a1 = a0[None, :, None], a1[None, :, None]
    h0 = img[sy0][:, sx0] * a0 + img[sy0][:, sx1] * a1
    h1 = img[sy1][:, sx0] * a0 + img[sy1][:, sx1] * a1
    return h0 * b0[:, None, None] + h1 * b1[:, None, None]


def inverse_entries(G):
    """(ig11, ig03, ig33, ig55) of the 6x6 moment matrix.  Its inverse splits into 1/G11, 1/G55 and the 3x3 block on
    (0, 3, 4) = [[a, b, b], [b, c, d], [b, d, c]], solved in closed form (the library does the same)."""
    a, b, c, d = G[0, 0], G[0, 3], G[3, 3], G[3, 4]
    det = a * (c + d) - 2 * b * b
    return 1.0 / G[1, 1], -b / det, 0.5 * (a / det + 1.0 / (c - d)), 1.0 / G[5, 5]


def poly_taps(dtype=np.float32):
    """FarnebackPrepareGaussian(7, 1.5): (g, xg, xxg) over -7..7 and (ig11, ig03, ig33, ig55) from the inverse of the 6x6
    moment matrix, which OpenCV accumulates in double from float32 products (float64 mode: all in float64)."""
    n, sigma = POLY_N, POLY_SIGMA
    xs = range(-n, n + 1)
    g = np.array([math.exp(-x * x / (2 * sigma * sigma)) for x in xs]).astype(dtype)
    s = 0.0
    for v in g:
        s += float(v)
    s = 1.0 / s
    g = np.array([float(v) * s for v in g]).astype(dtype)
    xg = np.array([dtype(x) * g[x + n] for x in xs], dtype)
    xxg = np.array([dtype(x * x) * g[x + n] for x in xs], dtype)
    G = np.zeros((6, 6))
    for y in xs:
        for x in xs:
            gg = g[y + n] * g[x + n]
            fx, fy = dtype(x), dtype(y)
            G[0, 0] += float(gg)
            G[1, 1] += float(gg * fx * fx)
            G[3, 3] += float(gg * fx * fx * fx * fx)
            G[5, 5] += float(gg * fx * fx * fy * fy)
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    return g, xg, xxg, inverse_entries(G)


def poly_exp(img, dtype=np.float32):
    """FarnebackPolyExp(n = 7, sigma = 1.5): [5, h, w] = (y, x, yy, xx, xy) coefficients."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_taps(dtype)
    n = POLY_N
    src = np.asarray(img, dtype)
    h, w = src.shape
    ys = np.arange(h)
    r0 = src * g[n]
    r1 = np.zeros_like(src)
    r2 = np.zeros_like(src)
    for k in range(1, n + 1):
        s0, s1 = src[np.maximum(ys - k, 0)], src[np.minimum(ys + k, h - 1)]
        p = s0 + s1
        r0 = r0 + g[n + k] * p
        r1 = r1 + xg[n + k] * (s1 - s0)
        r2 = r2 + xxg[n + k] * p
    xs = np.arange(w)
    f64 = np.float64
    b1 = (r0 * g[n]).astype(f64)
    b2 = np.zeros((h, w))
    b3 = (r1 * g[n]).astype(f64)
    b4 = np.zeros((h, w))
    b5 = (r2 * g[n]).astype(f64)
    b6 = np.zeros((h, w))
    for k in range(1, n + 1):
        R, L = np.minimum(xs + k, w - 1), np.maximum(xs - k, 0)
        tg = (r0[:, R] + r0[:, L]).astype(f64)
        b1 = b1 + tg * f64(g[n + k])
        b4 = b4 + tg * f64(xxg[n + k])
        b2 = b2 + ((r0[:, R] - r0[:, L]) * xg[n + k]).astype(f64)
        b3 = b3 + ((r1[:, R] + r1[:, L]) * g[n + k]).astype(f64)
        b6 = b6 + ((r1[:, R] - r1[:, L]) * xg[n + k]).astype(f64)
        b5 = b5 + ((r2[:, R] + r2[:, L]) * g[n + k]).astype(f64)
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55]).astype(dtype)


def update_matrices(R0, R1, flow, dtype=np.float32):
    """FarnebackUpdateMatrices: M [5, h, w] from R0, R1 [5, h, w] and flow [h, w, 2] (dx, dy)."""
    _, h, w = R0.shape
    one, half, quarter = dtype(1), dtype(0.5), dtype(0.25)
    dx, dy = flow[..., 0].astype(dtype), flow[..., 1].astype(dtype)
    X = np.broadcast_to(np.arange(w, dtype=dtype)[None, :], (h, w))
    Y = np.broadcast_to(np.arange(h, dtype=dtype)[:, None], (h, w))
    fx, fy = X + dx, Y + dy
    x1, y1 = np.floor(fx), np.floor(fy)
    fx, fy = fx - x1, fy - y1
    valid = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xi = np.where(valid, x1, 0).astype(np.int64)
    yi = np.where(valid, y1, 0).astype(np.int64)
    xj, yj = np.minimum(xi + 1, w - 1), np.minimum(yi + 1, h - 1)
    a00, a01 = (one - fx) * (one - fy), fx * (one - fy)
    a10, a11 = (one - fx) * fy, fx * fy
    r = [((a00 * R1[c][yi, xi] + a01 * R1[c][yi, xj]) + a10 * R1[c][yj, xi]) + a11 * R1[c][yj, xj] for c in range(5)]
    r2 = np.where(valid, r[0], dtype(0))
    r3 = np.where(valid, r[1], dtype(0))
    r4 = np.where(valid, (R0[2] + r[2]) * half, R0[2])
    r5 = np.where(valid, (R0[3] + r[3]) * half, R0[3])
    r6 = np.where(valid, (R0[4] + r[4]) * quarter, R0[4] * half)
    r2 = (R0[0] - r2) * half
    r3 = (R0[1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    bd = np.array(BORDER, dtype)
    B = len(BORDER)
    xs, ys = np.arange(w), np.arange(h)
    sx_lo = np.where(xs < B, bd[np.minimum(xs, B - 1)], one)
    sx_hi = np.where(xs >= w - B, bd[np.clip(w - xs - 1, 0, B - 1)], one)
    sy_lo = np.where(ys < B, bd[np.minimum(ys, B - 1)], one)
    sy_hi = np.where(ys >= h - B, bd[np.clip(h - ys - 1, 0, B - 1)], one)
    scale = ((sx_lo[None, :] * sx_hi[None, :]) * sy_lo[:, None]) * sy_hi[:, None]
    r2, r3, r4, r5, r6 = (v * scale for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3]).astype(dtype)


def window_taps(dtype=np.float32):
    """The 11-tap kernel of FarnebackUpdateFlow_GaussianBlur (sigma = 5 * 0.3), centre first: k[0..5]."""
    m = WINSIZE // 2
    sigma = m * 0.3
    k = [1.0]
    s = 1.0
    for i in range(1, m + 1):
        t = dtype(math.exp(-i * i / (2 * sigma * sigma)))
        k.append(float(t))
        s += float(t * dtype(2))
    s = 1.0 / s
    return np.array([v * s for v in k]).astype(dtype)


def blur_solve(M, dtype=np.float32):
    """FarnebackUpdateFlow_GaussianBlur without the matrix update: blur M vertically then horizontally (replicated border),
    solve each 2x2 system in double.  Returns the flow [h, w, 2] (dx, dy)."""
    k = window_taps(dtype)
    m = len(k) - 1
    _, h, w = M.shape
    ys, xs = np.arange(h), np.arange(w)
    v = M * k[0]
    for i in range(1, m + 1):
        v = v + (M[:, np.minimum(ys + i, h - 1)] + M[:, np.maximum(ys - i, 0)]) * k[i]
    s = v * k[0]
    for i in range(1, m + 1):
        s = s + k[i] * (v[:, :, np.maximum(xs - i, 0)] + v[:, :, np.minimum(xs + i, w - 1)])
    g11, g12, g22, h1, h2 = (s[c].astype(np.float64) for c in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1).astype(dtype)


def farneback(prev_u8, next_u8, dtype=np.float32):
    """calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 10, 2, 7, 1.5, OPTFLOW_FARNEBACK_GAUSSIAN): [H, W, 2] (dx, dy)."""
    prev_u8, next_u8 = np.asarray(prev_u8, np.uint8), np.asarray(next_u8, np.uint8)
    assert prev_u8.shape == next_u8.shape and prev_u8.ndim == 2
    flow = None
    for lv, width, height, ksize, sigma in level_table(*prev_u8.shape):
        if flow is None:
            flow = np.zeros((height, width, 2), dtype)
        else:
            flow = resize_linear(flow, width, height, dtype) * dtype(2)
        R0 = poly_exp(level_image(prev_u8, width, height, ksize, sigma, dtype), dtype)
        R1 = poly_exp(level_image(next_u8, width, height, ksize, sigma, dtype), dtype)
        M = update_matrices(R0, R1, flow, dtype)
        for it in range(ITERATIONS):
            flow = blur_solve(M, dtype)
            if it < ITERATIONS - 1:
                M = update_matrices(R0, R1, flow, dtype)
    return flow


def rint_flow(flow):
    """np.rint(flow).astype(int64), the reference's rounding (metric.py:274)."""
    return np.rint(np.asarray(flow)).astype(np.int64)


def warp_index(iflow, H, W):
    """The reference's transposed lookup (metric.py:287-294): the pixel (r, c) of frame i+1 is read at row
    clamp(c + dx, 0, H-1), column clamp(r + dy, 0, W-1).  iflow: int64 [H, W, 2] (dx, dy).  Returns flat indices [H, W]."""
    r, c = np.mgrid[:H, :W]
    row = np.clip(c + iflow[..., 0], 0, H - 1)
    col = np.clip(r + iflow[..., 1], 0, W - 1)
    return row * W + col


def messddt_pair(p0, t0, m0, p1, t1, m1, iflow):
    """(error, num) of one pair: sum |(p0-t0)^2 m0 - (p1w-t1w)^2 m1w| / 255^2 and sum(m0) + 1, exact (integer terms).
    Masks: {0,1} arrays or None (all pixels)."""
    H, W = np.asarray(t0).shape
    idx = warp_index(iflow, H, W)
    i64 = lambda a: np.asarray(a, np.int64)
    m0 = np.ones((H, W), np.int64) if m0 is None else (i64(m0) != 0).astype(np.int64)
    m1 = np.ones((H, W), np.int64) if m1 is None else (i64(m1) != 0).astype(np.int64)
    e0 = (i64(p0) - i64(t0)) ** 2 * m0
    e1 = ((i64(p1).ravel()[idx] - i64(t1).ravel()[idx]) ** 2) * m1.ravel()[idx]
    return int(np.abs(e0 - e1).sum()) / 255.0 ** 2, float(m0.sum()) + 1.0


def unknown_mask(t):
    """The reference's default mask 0 < target < 255 (metric.py:130-132)."""
    t = np.asarray(t)
    return ((t > 0) & (t < 255)).astype(np.uint8)


def messddt(pred, target, mask=None, flows=None, dtype=np.float64):
    """Per-pair (errors, nums) of a clip [B, H, W] of uint8 alphas, each pair (i, i+1) evaluated as the reference evaluates
    a two-frame batch, with the flow of (target[i], target[i+1]) (flows: optional precomputed [B-1, H, W, 2]).
    mask None: the reference's default."""
    pred, target = np.asarray(pred), np.asarray(target)
    if mask is None:
        mask = unknown_mask(target)
    errs, nums = [], []
    for i in range(len(target) - 1):
        f = farneback(target[i], target[i + 1], dtype) if flows is None else flows[i]
        e, n = messddt_pair(pred[i], target[i], mask[i], pred[i + 1], target[i + 1], mask[i + 1], rint_flow(f))
        errs.append(e)
        nums.append(n)
    return np.array(errs), np.array(nums)
