"""Numpy float32 restatements, operation by operation, of three per-frame glue kernels of csrc/glue.hip (built with fp contraction
off, so every float32 operation below is one rounded device operation): otvm_preprocess, the bilinear x4 of
otvm_upsample4_logits3 / otvm_upsample4_softmax3, and otvm_trimap_to_sm.  No GPU import: tests/test_glue_train_cpu.py holds them
to the oracle's statements and to F.interpolate, tests/test_gpu_glue.py holds the kernels to them bit for bit."""
import numpy as np

f32 = np.float32
IMG_SCALE = f32(1) / f32(255)                   # == np.float32(1.0 / 255): the kernel's 1.f / 255.f and the oracle's s = 1.0 / 255

# three (mean, std) sets of the shape the engine passes: the alpha network's, the query encoder's, the memory encoder's
NORMS = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
             mean_q=(0.471, 0.448, 0.408), std_q=(0.234, 0.239, 0.242),
             mean_m=(0.5, 0.25, 0.125), std_m=(0.5, 2.0, 0.3))


def composite(a, fg=None, bg=None, fg_u8=None, bg_u8=None, u8_rgb=False):
    """The composited RGB image [3, H, W] in [0, 1] (alpha/model.py:384-386).  a [H, W] float32; either fg / bg float32 BGR planes
    [3, H, W] in 0..255, or fg_u8 / bg_u8 uint8 [H, W, 3] in BGR (u8_rgb False) or RGB (True) order."""
    a = np.asarray(a, f32)
    out = np.empty((3,) + a.shape, f32)
    for c in range(3):
        if fg_u8 is not None:
            ch = c if u8_rgb else 2 - c
            sf = fg_u8[..., ch].astype(f32) * IMG_SCALE
            sb = bg_u8[..., ch].astype(f32) * IMG_SCALE
        else:
            sf = np.asarray(fg[2 - c], f32) * IMG_SCALE
            sb = np.asarray(bg[2 - c], f32) * IMG_SCALE
        out[c] = sf * a + sb * (f32(1) - a)
    return out


def preprocess(a, Hp, Wp, lh, lw, norms=NORMS, **src):
    """dict(scaled_imgs [3,H,W], imgp [3,Hp,Wp] zero padded, n / q / m [3,Hp,Wp] = (imgp - mean) / std for the three sets)."""
    img = composite(a, **src)
    H, W = img.shape[1:]
    imgp = np.zeros((3, Hp, Wp), f32)
    imgp[:, lh:lh + H, lw:lw + W] = img
    out = dict(scaled_imgs=img, imgp=imgp)
    for name, mk, sk in (("n", "mean", "std"), ("q", "mean_q", "std_q"), ("m", "mean_m", "std_m")):
        mean = np.asarray(norms[mk], f32).reshape(3, 1, 1)
        std = np.asarray(norms[sk], f32).reshape(3, 1, 1)
        out[name] = (imgp - mean) / std
    return out


def preprocess_lanes(r):
    """What the kernel stores per padded pixel, [P, lanes]: x11 lanes 0..3 = (n, 0), sq / sm lanes 0..3 = (q, 0) / (m, 0), d80 lanes
    64..69 = (n, img)."""
    P = r["imgp"].shape[1] * r["imgp"].shape[2]
    z = np.zeros((1, P), f32)
    flat = lambda k: r[k].reshape(3, P)
    return dict(x11=np.concatenate([flat("n"), z]).T.copy(), sq=np.concatenate([flat("q"), z]).T.copy(),
                sm=np.concatenate([flat("m"), z]).T.copy(), d80=np.concatenate([flat("n"), flat("imgp")]).T.copy())


def upsample4_logits(lg):
    """lg [3, h4, w4] float32 -> [3, 4 h4, 4 w4]: bilinear x4, align_corners False, with the kernel's coordinates and blend order
    hy (hx v00 + lx v01) + ly (hx v10 + lx v11)."""
    lg = np.asarray(lg, f32)
    _, h4, w4 = lg.shape

    def axis(n):
        f = (np.arange(4 * n).astype(f32) + f32(0.5)) * f32(0.25) - f32(0.5)
        f = np.where(f < 0, f32(0), f).astype(f32)
        i0 = f.astype(np.int64)
        i1 = i0 + (i0 < n - 1)
        lo = f - i0.astype(f32)
        return i0, i1, lo.astype(f32), (f32(1) - lo).astype(f32)
    y0, y1, ly, hy = axis(h4)
    x0, x1, lx, hx = axis(w4)
    ly, hy = ly[:, None], hy[:, None]
    top = hx * lg[:, y0][:, :, x0] + lx * lg[:, y0][:, :, x1]
    bot = hx * lg[:, y1][:, :, x0] + lx * lg[:, y1][:, :, x1]
    out = hy * top + ly * bot
    assert out.dtype == f32
    return out


def softmax3_f64(l):
    """float64 softmax over axis 0 of (restated, float32) logits [3, ...]."""
    l = np.asarray(l, np.float64)
    e = np.exp(l - l.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def trimap_to_sm(tri, sm):
    """tri [3, P] -> sm [P, ld] with lanes 3 / 4 = unknown / foreground; every other lane as it was."""
    out = np.array(sm, copy=True)
    out[:, 3] = tri[1]
    out[:, 4] = tri[2]
    return out
