"""numpy restatement of the video-stream kernels (include/otvm_hip.h: otvm_yuv_to_rgb, otvm_rgb_to_yuv420), operation by operation
with the same integers, and beside it their float64 DEFINITION: bilinear chroma at the stated siting, the standard's exact matrix,
round half up, clamp.  The restatement is what the GPU tests compare against bit for bit; the definition is what the restatement is
held to (tests/test_yuv_cpu.py), within one code value.

Why one: the luma coefficient is off by at most 2^-21 (times at most 239), a chroma coefficient by at most 2^-17 of a code value
per unit of 16 x chroma, i.e. 2^-21 per unit of an operand of at most 2048 -- together below 0.003 of a code value, far below the
1/2 that separates two roundings.  The interpolation weights are quarters, exact in both.  So the two can differ only where the
exact value lies within 0.003 of a tie, and then by one."""
import math

import numpy as np

SHIFT = 20
KR_KB = {"601": (0.299, 0.114), "709": (0.2126, 0.0722)}
LAYOUTS = ("420p", "nv12", "422p", "444p", "mono")
SUBSAMPLING = {"420p": (True, True), "nv12": (True, True), "422p": (True, False), "444p": (False, False), "mono": (False, False)}


def _rnd(x):
    return int(math.floor(x + 0.5))


def scales(rng):
    """(luma scale, chroma scale, luma offset) of a range."""
    return (219 / 255, 224 / 255, 16) if rng == "limited" else (1.0, 1.0, 0)


def inverse_constants(matrix, rng):
    """(CY, RV, GU, GV, BU) of otvm_yuv_to_rgb: 20 fractional bits; the chroma ones act on 16 x chroma, so they carry 2^16."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs, _ = scales(rng)
    return (_rnd((1 << SHIFT) / ys), _rnd(2 * (1 - kr) / cs * 65536), _rnd(2 * kb * (1 - kb) / kg / cs * 65536),
            _rnd(2 * kr * (1 - kr) / kg / cs * 65536), _rnd(2 * (1 - kb) / cs * 65536))


def forward_constants(matrix, rng):
    """(YR, YG, YB, CH, UR, VB) of otvm_rgb_to_yuv420.  YG is what is left of the range's scale, UG = CH - UR, VG = CH - VB: the
    luma weights sum to the scale exactly, the chroma rows to zero."""
    kr, kb = KR_KB[matrix]
    ys, cs, _ = scales(rng)
    one = _rnd(ys * (1 << SHIFT))
    yr, yb = _rnd(kr * ys * (1 << SHIFT)), _rnd(kb * ys * (1 << SHIFT))
    return (yr, one - yr - yb, yb, _rnd(0.5 * cs * (1 << SHIFT)), _rnd(kr / (2 * (1 - kb)) * cs * (1 << SHIFT)),
            _rnd(kb / (2 * (1 - kr)) * cs * (1 << SHIFT)))


def chroma_shape(H, W, layout):
    subx, suby = SUBSAMPLING[layout]
    return ((H + 1) // 2 if suby else H, (W + 1) // 2 if subx else W)


def _taps(n, nc, sub, centre):
    """Per luma position: two clamped chroma indices and their weights in quarters."""
    x = np.arange(n)
    if not sub:
        return x, x, np.full(n, 4), np.zeros(n, int)
    c, odd = x >> 1, (x & 1).astype(bool)
    if centre:
        a, b, wa, wb = c, np.where(odd, c + 1, c - 1), np.full(n, 3), np.full(n, 1)
    else:
        a, b, wa, wb = c, c + 1, np.where(odd, 2, 4), np.where(odd, 2, 0)
    return np.clip(a, 0, nc - 1), np.clip(b, 0, nc - 1), wa, wb


def chroma16(c, H, W, layout, siting, dtype=np.int64):
    """A chroma plane at luma resolution as 16 x chroma (exact in integers and in float64)."""
    subx, suby = SUBSAMPLING[layout]
    c = np.asarray(c).astype(dtype)
    xa, xb, wxa, wxb = _taps(W, c.shape[1], subx, siting == "centre")
    ya, yb, wya, wyb = _taps(H, c.shape[0], suby, True)               # 4:2:0 rows: always centre
    h = wxa[None, :].astype(dtype) * c[:, xa] + wxb[None, :].astype(dtype) * c[:, xb]
    return wya[:, None].astype(dtype) * h[ya] + wyb[:, None].astype(dtype) * h[yb]


def _split_uv(u, v, H, W, layout):
    if layout == "mono":
        return None, None
    if layout == "nv12":
        u = np.asarray(u).reshape(chroma_shape(H, W, layout) + (2,))
        return u[..., 0], u[..., 1]
    return np.asarray(u), np.asarray(v)


def yuv_to_rgb(y, u=None, v=None, layout="420p", matrix="601", rng="limited", siting="left", rgb=True):
    """The restatement of otvm_yuv_to_rgb -> uint8 [H,W,3]."""
    y = np.asarray(y).astype(np.int64)
    H, W = y.shape
    u, v = _split_uv(u, v, H, W, layout)
    if layout == "mono":
        du = dv = np.zeros((H, W), np.int64)
    else:
        du, dv = chroma16(u, H, W, layout, siting) - 2048, chroma16(v, H, W, layout, siting) - 2048
    cy, rv, gu, gv, bu = inverse_constants(matrix, rng)
    lum = cy * (y - scales(rng)[2]) + (1 << 19)
    R = np.clip((lum + rv * dv) >> SHIFT, 0, 255)
    G = np.clip((lum - gu * du - gv * dv) >> SHIFT, 0, 255)
    B = np.clip((lum + bu * du) >> SHIFT, 0, 255)
    assert max(np.abs(lum + rv * dv).max(), np.abs(lum - gu * du - gv * dv).max(), np.abs(lum + bu * du).max()) < 2 ** 31
    return np.stack([R, G, B] if rgb else [B, G, R], -1).astype(np.uint8)


def yuv_to_rgb_definition(y, u=None, v=None, layout="420p", matrix="601", rng="limited", siting="left", rgb=True):
    y = np.asarray(y).astype(np.float64)
    H, W = y.shape
    u, v = _split_uv(u, v, H, W, layout)
    if layout == "mono":
        cu = cv = np.zeros((H, W))
    else:
        cu = chroma16(u, H, W, layout, siting, np.float64) / 16 - 128
        cv = chroma16(v, H, W, layout, siting, np.float64) / 16 - 128
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs, yo = scales(rng)
    lum, cu, cv = (y - yo) / ys, cu / cs, cv / cs
    R = lum + 2 * (1 - kr) * cv
    B = lum + 2 * (1 - kb) * cu
    G = lum - (2 * kb * (1 - kb) / kg) * cu - (2 * kr * (1 - kr) / kg) * cv
    out = [np.clip(np.floor(c + 0.5), 0, 255) for c in ((R, G, B) if rgb else (B, G, R))]
    return np.stack(out, -1).astype(np.uint8)


def _block_sums(img):
    """[H,W,3] -> [ch,cw,3] sums over 2 x 2 blocks, coordinates clamped (an odd edge counts its last row / column twice)."""
    H, W = img.shape[:2]
    p = np.pad(img, ((0, H & 1), (0, W & 1), (0, 0)), mode="edge")
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def rgb_to_yuv420(img, matrix="601", rng="limited", rgb=True):
    """The restatement of otvm_rgb_to_yuv420 -> (y [H,W], u, v [ch,cw]) uint8."""
    img = np.asarray(img).astype(np.int64)
    if not rgb:
        img = img[..., ::-1]
    yr, yg, yb, ch, ur, vb = forward_constants(matrix, rng)
    yo = scales(rng)[2]
    R, G, B = img[..., 0], img[..., 1], img[..., 2]
    y = ((yr * R + yg * G + yb * B + (1 << 19)) >> SHIFT) + yo
    s = _block_sums(img)
    sR, sG, sB = s[..., 0], s[..., 1], s[..., 2]
    bias = (128 << 22) + (1 << 21)
    tu = -ur * sR - (ch - ur) * sG + ch * sB + bias
    tv = ch * sR - (ch - vb) * sG - vb * sB + bias
    assert 0 <= min(tu.min(), tv.min()) and max(tu.max(), tv.max()) < 2 ** 31
    return y.astype(np.uint8), np.clip(tu >> 22, 0, 255).astype(np.uint8), np.clip(tv >> 22, 0, 255).astype(np.uint8)


def rgb_to_yuv420_definition(img, matrix="601", rng="limited", rgb=True):
    img = np.asarray(img).astype(np.float64)
    if not rgb:
        img = img[..., ::-1]
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs, yo = scales(rng)

    def luma(p):
        return kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2]
    y = np.floor(yo + ys * luma(img) + 0.5)
    m = _block_sums(img) / 4
    u = np.floor(128 + cs * (m[..., 2] - luma(m)) / (2 * (1 - kb)) + 0.5)
    v = np.floor(128 + cs * (m[..., 0] - luma(m)) / (2 * (1 - kr)) + 0.5)
    return tuple(np.clip(p, 0, 255).astype(np.uint8) for p in (y, u, v))


def pack_frame(y, u=None, v=None, layout="420p"):
    """The planes as one contiguous Y4M frame (bytes); nv12: u is the interleaved plane."""
    parts = [np.ascontiguousarray(y, np.uint8).tobytes()]
    if layout == "nv12":
        parts.append(np.ascontiguousarray(u, np.uint8).tobytes())
    elif layout != "mono":
        parts += [np.ascontiguousarray(u, np.uint8).tobytes(), np.ascontiguousarray(v, np.uint8).tobytes()]
    return b"".join(parts)


def split_frame(buf, H, W, layout):
    """The inverse of pack_frame -> (y, u, v) arrays (nv12: (y, uv [ch,cw,2], None); mono: (y, None, None))."""
    a = np.frombuffer(buf, np.uint8)
    y = a[:H * W].reshape(H, W)
    if layout == "mono":
        return y, None, None
    ch, cw = chroma_shape(H, W, layout)
    if layout == "nv12":
        return y, a[H * W:H * W + ch * cw * 2].reshape(ch, cw, 2), None
    n = ch * cw
    return y, a[H * W:H * W + n].reshape(ch, cw), a[H * W + n:H * W + 2 * n].reshape(ch, cw)


def random_planes(rng_, H, W, layout, corners=False):
    """(y, u, v) test planes: uniform bytes, or drawn from the range corners 0 / 16 / 128 / 235 / 240 / 255."""
    def draw(shape):
        if corners:
            return rng_.choice(np.array([0, 16, 128, 235, 240, 255], np.uint8), size=shape)
        return rng_.integers(0, 256, size=shape, dtype=np.uint8)
    y = draw((H, W))
    if layout == "mono":
        return y, None, None
    ch, cw = chroma_shape(H, W, layout)
    if layout == "nv12":
        return y, draw((ch, cw, 2)), None
    return y, draw((ch, cw)), draw((ch, cw))
