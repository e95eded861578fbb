"""numpy restatement of the temporal stabilisation of alpha (include/otvm_hip.h: otvm_luma_u8, otvm_temporal_blend; the chain
of otvm_amd/temporal.py): every step one float32 IEEE operation, in the kernel's order.  TEST INFRASTRUCTURE, shared by
tests/test_temporal_ref.py (CPU) and tests/test_gpu_temporal.py.

The clamps and the two ramps are written as selects (v > 0 ? v : 0, v < 1 ? v : 1), which is fmaxf / fminf for every value
and leaves no choice for -0.0 or NaN: the outputs are compared bit for bit."""
import numpy as np

F32 = np.float32


def luma_u8(img, rgb=False):
    """uint8 [H,W,3] (B,G,R unless ``rgb``) -> uint8 [H,W]: (B*1868 + G*9617 + R*4899 + 8192) >> 14, OpenCV's BGR2GRAY."""
    x = np.asarray(img).astype(np.int32)
    b, g, r = (x[..., 2], x[..., 1], x[..., 0]) if rgb else (x[..., 0], x[..., 1], x[..., 2])
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def _ramp(v):
    """fmaxf(0, v) as a select (NaN gives 0)"""
    return np.where(v > 0, v, F32(0.0)).astype(F32)


def clamp01(v):
    v = np.asarray(v, F32)
    lo = np.where(v > 0, v, F32(0.0)).astype(F32)
    return np.where(lo < 1, lo, F32(1.0)).astype(F32)


def quant_u8(out):
    """(uint8) trunc(out * 255) of a clamped plane; a non-finite value gives 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.trunc(np.asarray(out, F32) * F32(255.0))
    return np.where(np.isfinite(out), t, F32(0.0)).astype(np.uint8)


def finish(alpha, o):
    """(out, out_u8) of the unclamped result ``o``: clamped, a non-finite alpha passes through with byte 0"""
    fin = np.isfinite(alpha)
    out = np.where(fin, clamp01(o), alpha).astype(F32)
    return out, np.where(fin, quant_u8(np.where(fin, out, F32(0.0))), 0).astype(np.uint8)


def first(alpha):
    """The first step of a clip: the clamped input and its byte."""
    alpha = np.asarray(alpha, F32)
    return finish(alpha, alpha)


def sample(plane, sx, sy, ok):
    """Bilinear sample of ``plane`` (any dtype, converted to float32) at (sx, sy) where ``ok``; 0 elsewhere (never used)."""
    H, W = plane.shape
    with np.errstate(invalid="ignore", over="ignore"):
        fx0, fy0 = np.floor(sx), np.floor(sy)
        fx, fy = (sx - fx0).astype(F32), (sy - fy0).astype(F32)
        x0 = np.minimum(np.where(ok, fx0, 0).astype(np.int64), W - 1)
        y0 = np.minimum(np.where(ok, fy0, 0).astype(np.int64), H - 1)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    p = plane.astype(F32)
    v00, v01, v10, v11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    one = F32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = ((one - fx) * v00).astype(F32) + (fx * v01).astype(F32)
        bot = ((one - fx) * v10).astype(F32) + (fx * v11).astype(F32)
        v = ((one - fy) * top).astype(F32) + (fy * bot).astype(F32)
    return np.where(ok, v, F32(0.0)).astype(F32)


def gate_of(tri, H, W, tri_scale):
    """1 where numpy's first-max argmax of the trimap at (min(y / s, th-1), min(x / s, tw-1)) is 1 (NaN gives 0)"""
    if tri is None:
        return np.ones((H, W), F32)
    tri = np.asarray(tri, F32)
    th, tw = tri.shape[1:]
    yy = np.minimum(np.arange(H) // tri_scale, th - 1)[:, None]
    xx = np.minimum(np.arange(W) // tri_scale, tw - 1)[None, :]
    t0, t1, t2 = tri[0][yy, xx], tri[1][yy, xx], tri[2][yy, xx]
    with np.errstate(invalid="ignore"):
        return ((t1 > t0) & (t1 >= t2)).astype(F32)


def blend(alpha, prev, grey, grey_prev, flow, tri=None, tri_scale=1, strength=0.5, inv_tau_colour=None, inv_tau_alpha=None,
          tau_colour=24.0, tau_alpha=0.5):
    """otvm_temporal_blend.  The reciprocals default to float32(1) / float32(tau), as the host takes them."""
    alpha, prev, flow = np.asarray(alpha, F32), np.asarray(prev, F32), np.asarray(flow, F32)
    H, W = alpha.shape
    k = F32(strength)
    itc = F32(1.0) / F32(tau_colour) if inv_tau_colour is None else F32(inv_tau_colour)
    ita = F32(1.0) / F32(tau_alpha) if inv_tau_alpha is None else F32(inv_tau_alpha)
    one = F32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (np.arange(W, dtype=F32)[None, :] + flow[..., 0]).astype(F32)
        sy = (np.arange(H, dtype=F32)[:, None] + flow[..., 1]).astype(F32)
        ok = (sx >= 0) & (sx <= F32(W - 1)) & (sy >= 0) & (sy <= F32(H - 1))
        sw = sample(prev, sx, sy, ok)
        gw = sample(np.asarray(grey_prev), sx, sy, ok)
        wc = _ramp(one - (np.abs(np.asarray(grey).astype(F32) - gw) * itc).astype(F32))
        wa = _ramp(one - (np.abs(alpha - sw) * ita).astype(F32))
        w = (((k * wc).astype(F32) * wa).astype(F32) * gate_of(tri, H, W, tri_scale)).astype(F32)
        w = np.where(ok, w, F32(0.0)).astype(F32)
        o = (alpha + (w * (sw - alpha)).astype(F32)).astype(F32)
    return finish(alpha, o)


def chain(frames, raws, flows, tris=None, tri_scale=1, rgb=False, **kw):
    """The stabiliser's chain over a clip: flows[t] (t >= 1) is the flow from frame t to frame t-1, [H,W,2].
    Returns the stabilised alphas [T,H,W] and their bytes."""
    outs, u8s, prev, gp = [], [], None, None
    for t, (f, a) in enumerate(zip(frames, raws)):
        g = luma_u8(f, rgb)
        if t == 0:
            o, b = first(a)
        else:
            o, b = blend(a, prev, g, gp, np.asarray(flows[t], F32), None if tris is None else tris[t], tri_scale, **kw)
        outs.append(o), u8s.append(b)
        prev, gp = o, g
    return np.stack(outs), np.stack(u8s)


# ------------------------------------------------------------------------------------------------ the synthetic clips
CLIPS = [(64, 96, (2, 1), 0), (64, 96, (3, -1), 1), (96, 128, (1, 2), 2)]      # (H, W, v, seed)
T_CLIP, SIGMA = 6, 0.08


def smooth(rng, H, W, n):
    x = rng.random((H + 8, W + 8))
    for _ in range(n):
        x = (x + np.roll(x, 1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 0) + np.roll(x, -1, 1)) / 5
    x = (x - x.min()) / (x.max() - x.min())
    return x[4:-4, 4:-4]


def clip(H, W, T, v, seed, sigma):
    """A textured disc moving by v = (vx, vy) per frame over a textured background: (frames in B,G,R order, ground-truth
    alphas, raw alphas = the ground truth with noise in the band)."""
    rng = np.random.default_rng(seed)
    bg = np.stack([smooth(rng, H, W, 2) for _ in range(3)], -1) * 0.5
    big = np.stack([smooth(rng, 3 * H, 3 * W, 2) for _ in range(3)], -1) * 0.5 + 0.5
    ys, xs = np.mgrid[0:H, 0:W]
    frames, gts, raws = [], [], []
    for t in range(T):
        d = np.sqrt((xs - (W * 0.35 + v[0] * t)) ** 2 + (ys - (H * 0.4 + v[1] * t)) ** 2)
        gt = np.clip((H * 0.28 - d) / 6.0 + 0.5, 0, 1)
        fg = big[H - v[1] * t: 2 * H - v[1] * t, W - v[0] * t: 2 * W - v[0] * t]
        frames.append(((fg * gt[..., None] + bg * (1 - gt[..., None])) * 255).astype(np.uint8))
        gts.append(gt.astype(np.float32))
        raws.append(np.clip(gt + ((gt > 0) & (gt < 1)) * rng.normal(0, sigma, gt.shape), 0, 1).astype(np.float32))
    return frames, gts, raws


def translated(H, W, T, v, seed):
    """Whole-frame translations of the clip generator's foreground texture by v per frame (B,G,R uint8 frames)."""
    rng = np.random.default_rng(seed)
    [smooth(rng, H, W, 2) for _ in range(3)]                       # (the generator's background comes first in its stream)
    big = np.stack([smooth(rng, 3 * H, 3 * W, 2) for _ in range(3)], -1) * 0.5 + 0.5
    return [(big[H - v[1] * t: 2 * H - v[1] * t, W - v[0] * t: 2 * W - v[0] * t] * 255).astype(np.uint8) for t in range(T)]


def trimaps_of(gts):
    """one-hot [3,H,W] per frame: bg where gt == 0, fg where gt == 1, otherwise unknown"""
    return [np.stack([g == 0, (g > 0) & (g < 1), g == 1]).astype(np.float32) for g in gts]


def dtssd(p, gt):
    p, gt = np.asarray(p, np.float64), np.asarray(gt, np.float64)
    return float(sum(np.sqrt((((p[t] - p[t - 1]) - (gt[t] - gt[t - 1])) ** 2).sum()) for t in range(1, len(p))))


def sad(p, gt):
    return float(np.abs(np.asarray(p, np.float64) - np.asarray(gt, np.float64)).sum())


def ratios(stab, raws, gts):
    """(dtSSD ratio, SAD ratio) of the stabilised clip to the raw one, whole frames"""
    return dtssd(stab, gts) / dtssd(raws, gts), sad(stab, gts) / sad(raws, gts)


_CACHE = {}


def clip_case(idx, dtype=np.float32):
    """Clip ``idx`` of CLIPS with everything the tests share, computed once per process and never modified: frames, gts, raws,
    tris, greys and the restated flows (tests/farneback_ref.farneback(grey_t, grey_{t-1}) in ``dtype``; entry 0 is None)."""
    from tests import farneback_ref as FB
    key = (idx, np.dtype(dtype).name)
    if key not in _CACHE:
        base = _CACHE.get((idx, "base"))
        if base is None:
            H, W, v, seed = CLIPS[idx]
            frames, gts, raws = clip(H, W, T_CLIP, v, seed, SIGMA)
            base = _CACHE[(idx, "base")] = dict(frames=frames, gts=gts, raws=raws, tris=trimaps_of(gts),
                                                greys=[luma_u8(f) for f in frames], v=v)
        g = base["greys"]
        flows = [None] + [np.asarray(FB.farneback(g[t], g[t - 1], dtype)) for t in range(1, len(g))]
        _CACHE[key] = dict(base, flows=flows)
    return _CACHE[key]
