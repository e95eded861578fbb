"""Restatement of otvm_trimap_from_mask (include/otvm_hip.h) in numpy, integers only.

    FG = (m >= hi), BG = (m <= lo) for a uint8 mask m [H,W], 0 <= lo < hi <= 255;
    d_S(p) = min over the in-image pixels q not in S of |p - q|^2 (+inf when every pixel is in S; pixels outside the image belong
    to no set and seed nothing);
    fg = FG and d_FG > t_fg, bg = BG and d_BG > t_bg, everything else unknown; t = floor(r^2) for a band of r pixels.

``brute`` is that definition, pair by pair.  ``capped`` is the bounded separable form -- vertical distance to the nearest
non-member capped at R + 1, R = floor(sqrt(t)), then per row the minimum over |dx| <= R of g^2 + dx^2 -- which the CPU tests hold
against the definition and which serves as the yardstick at large sizes.  Both return the class map uint8 [H,W]: 0 bg, 1 unknown,
2 fg."""
import math

import numpy as np


def band_t(r):
    """t = floor(r^2) of a real radius r in 0 ... 255."""
    return int(math.floor(float(r) * float(r)))


def quantise(mask):
    """A float mask in [0,1] -> uint8 as otvm_amd.masks.quantise does (fp32: clamp, * 255, + 0.5, truncate)."""
    m = np.asarray(mask)
    if m.dtype == np.uint8:
        return m
    m = np.clip(m.astype(np.float32), np.float32(0), np.float32(1))
    return (m * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def _keep_brute(S, t):
    """S and d_S > t, from the definition."""
    H, W = S.shape
    out = np.zeros((H, W), bool)
    qy, qx = np.nonzero(~S)
    py, px = np.nonzero(S)
    if qy.size == 0:
        return S.copy()                                   # no pixel outside the set: d = +inf everywhere
    qy, qx, py, px = (a.astype(np.int64) for a in (qy, qx, py, px))
    for s in range(0, py.size, 512):
        dy = py[s:s + 512, None] - qy[None, :]
        dx = px[s:s + 512, None] - qx[None, :]
        d = (dy * dy + dx * dx).min(1)
        out[py[s:s + 512], px[s:s + 512]] = d > t
    return out


def _keep_capped(S, t):
    """S and d_S > t by the bounded separable search."""
    H, W = S.shape
    R = math.isqrt(int(t))
    cap = R + 1
    g = np.zeros((H, W), np.int64)
    d = np.full(W, cap, np.int64)                         # above the image: nothing
    for y in range(H):
        d = np.where(S[y], np.minimum(d + 1, cap), 0)
        g[y] = d
    d = np.full(W, cap, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(S[y], np.minimum(d + 1, cap), 0)
        g[y] = np.minimum(g[y], d)
    g2 = g * g
    far = np.int64(1) << 40
    pad = np.full((H, W + 2 * R), far, np.int64)          # beside the image: nothing
    pad[:, R:R + W] = g2
    best = np.full((H, W), far, np.int64)
    for dx in range(-R, R + 1):
        best = np.minimum(best, pad[:, R + dx:R + dx + W] + dx * dx)
    return S & (best > t)


def classes(mask, lo, hi, t_fg, t_bg, brute=False):
    """uint8 mask [H,W] -> class map uint8 [H,W] (0 bg, 1 unknown, 2 fg)."""
    m = np.asarray(mask)
    assert m.dtype == np.uint8 and m.ndim == 2 and 0 <= lo < hi <= 255 and t_fg >= 0 and t_bg >= 0
    keep = _keep_brute if brute else _keep_capped
    fg, bg = keep(m >= hi, int(t_fg)), keep(m <= lo, int(t_bg))
    out = np.ones(m.shape, np.uint8)
    out[bg] = 0
    out[fg] = 2
    return out


def onehot(cls):
    """class map -> planar one-hot float32 [3,H,W] (bg, unknown, fg)."""
    return np.stack([(cls == k) for k in range(3)]).astype(np.float32)


def label_map(cls, band_label):
    """class map -> uint8 label map: 0 bg, 2 fg, ``band_label`` (1 or 255) in the band."""
    out = cls.copy()
    out[cls == 1] = band_label
    return out


def trimap_from_mask(mask, band, lo=127, hi=128):
    """What otvm_amd.masks.trimap_from_mask returns without ``labels``: the one-hot trimap of a uint8 / float mask, band = r or
    (r_fg, r_bg)."""
    r_fg, r_bg = band if isinstance(band, (tuple, list)) else (band, band)
    return onehot(classes(quantise(mask), lo, hi, band_t(r_fg), band_t(r_bg)))


def labels_from_mask(mask, band, lo=127, hi=128, band_label=255):
    r_fg, r_bg = band if isinstance(band, (tuple, list)) else (band, band)
    return label_map(classes(quantise(mask), lo, hi, band_t(r_fg), band_t(r_bg)), band_label)
