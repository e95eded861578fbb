"""numpy restatement of working-resolution matting (include/otvm_hip.h: otvm_downsample_*, otvm_guided_coeffs, otvm_guided_apply),
written from the definition: the reductions in integers, the coefficient algebra and the box mean in float64 in the stated
order, the apply in float32 with one IEEE operation per step.  ``bilinear_upsample`` is the plain upsampler with the same
sampling rule (what the guided filter is compared against)."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64


def work_size(H, W, s):
    return (H + s - 1) // s, (W + s - 1) // s


def _blocks(H, W, s):
    h, w = work_size(H, W, s)
    for y in range(h):
        for x in range(w):
            yield y, x, slice(y * s, min(y * s + s, H)), slice(x * s, min(x * s + s, W))


# ------------------------------------------------------------------------------------------------ reductions
def downsample_u8(img, s):
    """uint8 [H,W,3] -> [h,w,3]: (sum + n // 2) // n over the clipped s x s block of n pixels."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    h, w = work_size(H, W, s)
    pad = np.zeros((h * s, w * s, 3), I64)
    pad[:H, :W] = img
    cnt = np.zeros((h * s, w * s), I64)
    cnt[:H, :W] = 1
    sums = pad.reshape(h, s, w, s, 3).sum((1, 3))
    n = cnt.reshape(h, s, w, s).sum((1, 3))[..., None]
    return ((sums + n // 2) // n).astype(np.uint8)


def downsample_trimap(tri, s):
    """one-hot float [3,H,W] -> [3,h,w]: fg (bg) only if plane 2 (0) is 1.0 on every pixel of the block, else unknown."""
    tri = np.asarray(tri, F32)
    _, H, W = tri.shape
    h, w = work_size(H, W, s)
    out = np.zeros((3, h, w), F32)
    for y, x, ys, xs in _blocks(H, W, s):
        all_bg, all_fg = bool((tri[0, ys, xs] == 1).all()), bool((tri[2, ys, xs] == 1).all())
        fg, bg = all_fg and not all_bg, all_bg and not all_fg
        out[:, y, x] = (1, 0, 0) if bg else ((0, 0, 1) if fg else (0, 1, 0))
    return out


def downsample_labels(lab, s):
    """uint8 [H,W] -> [h,w]: 255 if any pixel of the block is no class (> 2), the common class, otherwise 1."""
    lab = np.asarray(lab, np.uint8)
    H, W = lab.shape
    h, w = work_size(H, W, s)
    out = np.zeros((h, w), np.uint8)
    for y, x, ys, xs in _blocks(H, W, s):
        b = lab[ys, xs]
        out[y, x] = 255 if (b > 2).any() else (b.flat[0] if (b == b.flat[0]).all() else 1)
    return out


# ------------------------------------------------------------------------------------------------ coefficients
def quantise(p):
    p = np.asarray(p, F32)
    return (np.fmin(np.fmax(p, F32(0)), F32(1)) * F32(65535.0) + F32(0.5)).astype(np.int32).astype(I64)


def _window_sum_int(a, r):
    """exact integer sum over the clipped (2r+1)^2 window (order-free)."""
    h, w = a.shape
    c = np.zeros((h + 1, w + 1), I64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def window_count(h, w, r):
    return _window_sum_int(np.ones((h, w), I64), r)


def guided_coeffs_raw(guide, targets, r, eps):
    """guide uint8 [h,w,3], targets [C,h,w] float32 -> raw (a0, a1, a2, b) float32 [h,w,C,4]."""
    I = np.asarray(guide, np.uint8).astype(I64)
    h, w = I.shape[:2]
    N = window_count(h, w, r)
    S = [_window_sum_int(I[..., c], r) for c in range(3)]
    SS = {(c, d): _window_sum_int(I[..., c] * I[..., d], r) for c in range(3) for d in range(c, 3)}
    dI, dP, dn = (N * N * 65025).astype(F64), (N * N * 255 * 65535).astype(F64), N.astype(F64)
    eps = F64(eps)
    sig = {k: (N * SS[k] - S[k[0]] * S[k[1]]).astype(F64) / dI for k in SS}
    s00, s01, s02, s11, s12, s22 = sig[0, 0] + eps, sig[0, 1], sig[0, 2], sig[1, 1] + eps, sig[1, 2], sig[2, 2] + eps
    c00 = s11 * s22 - s12 * s12
    c01 = s02 * s12 - s01 * s22
    c02 = s01 * s12 - s02 * s11
    c11 = s00 * s22 - s02 * s02
    c12 = s01 * s02 - s00 * s12
    c22 = s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    m = [(S[c].astype(F64) / dn) / F64(255.0) for c in range(3)]
    out = np.zeros((h, w, len(targets), 4), F32)
    for t, tgt in enumerate(targets):
        P = quantise(tgt)
        SP = _window_sum_int(P, r)
        p = [(N * _window_sum_int(I[..., c] * P, r) - S[c] * SP).astype(F64) / dP for c in range(3)]
        a0 = ((c00 * p[0] + c01 * p[1]) + c02 * p[2]) / det
        a1 = ((c01 * p[0] + c11 * p[1]) + c12 * p[2]) / det
        a2 = ((c02 * p[0] + c12 * p[1]) + c22 * p[2]) / det
        mP = (SP.astype(F64) / dn) / F64(65535.0)
        b = mP - ((a0 * m[0] + a1 * m[1]) + a2 * m[2])
        out[:, :, t] = np.stack([a0, a1, a2, b], -1).astype(F32)
    return out


def box_mean(raw, r):
    """float32 [h,w,...] -> box mean over the clipped window in float64: rows summed in ascending x, then columns in ascending
    y (each sum starts from 0.0), divided by N, rounded to float32."""
    raw = np.asarray(raw, F32)
    h, w = raw.shape[:2]
    v = raw.astype(F64)
    rows = np.zeros_like(v)
    for x in range(w):
        acc = np.zeros_like(v[:, 0])
        for xx in range(max(x - r, 0), min(x + r, w - 1) + 1):
            acc = acc + v[:, xx]
        rows[:, x] = acc
    cols = np.zeros_like(v)
    for y in range(h):
        acc = np.zeros_like(v[0])
        for yy in range(max(y - r, 0), min(y + r, h - 1) + 1):
            acc = acc + rows[yy]
        cols[y] = acc
    N = window_count(h, w, r).astype(F64).reshape((h, w) + (1,) * (raw.ndim - 2))
    return (cols / N).astype(F32)


def guided_coeffs(guide, targets, r, eps):
    raw = guided_coeffs_raw(guide, targets, r, eps)
    return raw, box_mean(raw, r)


# ------------------------------------------------------------------------------------------------ apply
def sample_positions(n_full, s, n_work):
    """half-pixel centres in integers: (i0, i1, f) per full-resolution index."""
    X = np.arange(n_full, dtype=I64)
    t = 2 * X + 1 - s
    q = np.floor_divide(t, 2 * s)
    f = (t - 2 * s * q).astype(F32) / F32(2 * s)
    return np.clip(q, 0, n_work - 1), np.clip(q + 1, 0, n_work - 1), f.astype(F32)


def _bilinear(planes, H, W, s):
    """planes float32 [h,w,...] -> [H,W,...]: top = c00 + fx (c01 - c00), bot alike, v = top + fy (bot - top), all float32."""
    planes = np.asarray(planes, F32)
    h, w = planes.shape[:2]
    ya, yb, fy = sample_positions(H, s, h)
    xa, xb, fx = sample_positions(W, s, w)
    ex = (1,) * (planes.ndim - 2)
    fx = fx.reshape((1, W) + ex)
    fy = fy.reshape((H, 1) + ex)
    c00, c01 = planes[ya][:, xa], planes[ya][:, xb]
    c10, c11 = planes[yb][:, xa], planes[yb][:, xb]
    top = c00 + fx * (c01 - c00)
    bot = c10 + fx * (c11 - c10)
    out = top + fy * (bot - top)
    assert out.dtype == F32
    return out


def bilinear_upsample(plane, H, W, s):
    return _bilinear(plane, H, W, s)


def _clamp01(q):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(q), F32(0), np.where(q < F32(0), F32(0), np.where(q > F32(1), F32(1), q))).astype(F32)


def guided_apply(frame, coef, s):
    """frame uint8 [H,W,3], coef float32 [h,w,C,4] -> (alpha [H,W] float32, alpha_u8 [H,W], fgr [3,H,W] float32 or None)."""
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape[:2]
    v = _bilinear(coef, H, W, s)                                    # [H,W,C,4]
    I = frame.astype(F32) * (F32(1.0) / F32(255.0))
    outs = []
    for c in range(coef.shape[2]):
        q = ((v[:, :, c, 0] * I[..., 0] + v[:, :, c, 1] * I[..., 1]) + v[:, :, c, 2] * I[..., 2]) + v[:, :, c, 3]
        assert q.dtype == F32
        outs.append(_clamp01(q))
    alpha = outs[0]
    u8 = (alpha * F32(255.0)).astype(np.uint8)                      # truncation, as otvm_crop_outputs
    return alpha, u8, (np.stack(outs[1:4]) if len(outs) == 4 else None)


def guided_upsample(frame, work_frame, targets, s, r, eps):
    _, coef = guided_coeffs(work_frame, targets, r, eps)
    return guided_apply(frame, coef, s)
