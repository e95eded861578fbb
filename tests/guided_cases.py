"""Inputs shared by the CPU and GPU tests of working-resolution matting (tests/guided_ref.py is the arithmetic)."""
import numpy as np

from tests import guided_ref as R


def edge_case(H=96, W=128, s=2, seed=5):
    """A two-colour step image with noise whose edge is not aligned to the s grid (a slanted line through odd columns): the true
    alpha is the step, the working alpha its block mean.  Returns (frame u8 [H,W,3], true alpha f32 [H,W], working frame,
    working alpha f32 [h,w])."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    true = (xx > W // 2 + 1 + yy // 7).astype(np.float32)
    fg_col, bg_col = np.array([200.0, 60.0, 40.0]), np.array([30.0, 90.0, 180.0])
    img = true[..., None] * fg_col + (1 - true[..., None]) * bg_col + g.normal(0, 4.0, (H, W, 3))
    frame = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    h, w = R.work_size(H, W, s)
    pad = np.zeros((h * s, w * s), np.float64)
    cnt = np.zeros((h * s, w * s), np.float64)
    pad[:H, :W], cnt[:H, :W] = true, 1
    work_alpha = (pad.reshape(h, s, w, s).sum((1, 3)) / cnt.reshape(h, s, w, s).sum((1, 3))).astype(np.float32)
    return frame, true, R.downsample_u8(frame, s), work_alpha


def solid_case(H=73, W=105, s=3, seed=8):
    """A noisy frame and a working alpha with solid 0 / 1 regions around a soft band.  Returns (frame, working frame, alpha)."""
    g = np.random.default_rng(seed)
    frame = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    h, w = R.work_size(H, W, s)
    xx = np.arange(w, dtype=np.float32)[None, :] + np.zeros((h, 1), np.float32)
    alpha = np.clip((xx - w * 0.45) / 3.0, 0, 1).astype(np.float32)
    alpha[: h // 4, : w // 3] = 1.0                       # a solid island inside the zero side
    return frame, R.downsample_u8(frame, s), alpha


def solid_mask(alpha_w, value, H, W, s, reach):
    """Full-resolution pixels all of whose four bilinear neighbours see only ``value`` within ``reach`` working pixels."""
    h, w = alpha_w.shape
    ok = (alpha_w == value).astype(np.int64)
    full = R._window_sum_int(ok, reach) == R.window_count(h, w, reach)
    ya, yb, _ = R.sample_positions(H, s, h)
    xa, xb, _ = R.sample_positions(W, s, w)
    return full[ya][:, xa] & full[ya][:, xb] & full[yb][:, xa] & full[yb][:, xb]
