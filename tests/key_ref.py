"""The masks of keyed footage, twice (numpy only, no GPU):

  * the RESTATEMENT of otvm_mask_from_chroma and otvm_mask_from_plate with the kernels' own integers (include/otvm_hip.h) -- what
    the GPU tests compare bit for bit;
  * the float64 DEFINITION -- exact BT.601 full-range Cb, Cr, round half up, clamp; the cone quantity and the ramps in exact
    arithmetic; the plate distance by brute force over the neighbourhood -- which tests/test_key_cpu.py holds the restatement to.

Masks: 255 subject, 0 screen / plate."""
import math

import numpy as np

CH, UR, VB = 524288, 176932, 85262                  # BT.601 full range chroma rows, 20 fractional bits; UG = CH - UR, VG = CH - VB
KR_, KB_ = 0.299, 0.114                             # the standard's luma weights


# ------------------------------------------------------------------------------------------------ restatement
def chroma_int(R, G, B):
    """(cb, cr) = (Cb - 128, Cr - 128) as the kernel makes them, int64 arrays of the inputs' shape"""
    R, G, B = (np.asarray(v).astype(np.int64) for v in (R, G, B))
    bias = (128 << 20) + (1 << 19)
    cb = np.clip((-UR * R - (CH - UR) * G + CH * B + bias) >> 20, 0, 255) - 128
    cr = np.clip((CH * R - (CH - VB) * G - VB * B + bias) >> 20, 0, 255) - 128
    return cb, cr


def key_chroma(colour):
    cb, cr = chroma_int(*colour)
    return int(cb), int(cr)


def thresholds(kb, kr, lo, hi):
    """(qlo, qhi) = round half up of lo |K|, hi |K| in float64: the one floating-point step, made once per clip on the host"""
    norm = math.sqrt(float(kb * kb + kr * kr))
    return int(math.floor(float(lo) * norm + 0.5)), int(math.floor(float(hi) * norm + 0.5))


def cone(cb, cr, kb, kr):
    cb, cr = np.asarray(cb).astype(np.int64), np.asarray(cr).astype(np.int64)
    return cb * kb + cr * kr - np.abs(cb * kr - cr * kb)


def ramp_down(q, qlo, qhi):
    """255 where q <= qlo, 0 where q >= qhi, 255 - ((q - qlo) 255) // (qhi - qlo) between"""
    q = np.asarray(q).astype(np.int64)
    mid = 255 - ((np.clip(q, qlo, qhi) - qlo) * 255) // (qhi - qlo)
    return np.where(q <= qlo, 255, np.where(q >= qhi, 0, mid)).astype(np.uint8)


def ramp_up(d, lo, hi):
    """0 where d <= lo, 255 where d >= hi, ((d - lo) 255) // (hi - lo) between"""
    d = np.asarray(d).astype(np.int64)
    mid = ((np.clip(d, lo, hi) - lo) * 255) // (hi - lo)
    return np.where(d <= lo, 0, np.where(d >= hi, 255, mid)).astype(np.uint8)


def split(frame, rgb):
    f = np.asarray(frame)
    return (f[..., 0], f[..., 1], f[..., 2]) if rgb else (f[..., 2], f[..., 1], f[..., 0])


def chroma_q(frame, kb, kr, rgb=False):
    return cone(*chroma_int(*split(frame, rgb)), kb, kr)


def mask_from_chroma(frame, kb, kr, qlo, qhi, rgb=False):
    """otvm_mask_from_chroma: frame uint8 [H,W,3] -> uint8 [H,W]"""
    return ramp_down(chroma_q(frame, kb, kr, rgb), qlo, qhi)


def plate_distance(frame, plate, radius):
    """d [H,W] int64: min over the (2r+1)^2 neighbourhood of the PLATE (edge-clamped) of max_c |I_c - P_c|, by shifted planes"""
    f = np.asarray(frame).astype(np.int64)
    H, W = f.shape[:2]
    pp = np.pad(np.asarray(plate).astype(np.int64), ((radius, radius), (radius, radius), (0, 0)), mode="edge")
    d = np.full((H, W), 255, np.int64)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            d = np.minimum(d, np.abs(f - pp[dy:dy + H, dx:dx + W]).max(-1))
    return d


def mask_from_plate(frame, plate, radius, lo, hi):
    """otvm_mask_from_plate: frame, plate uint8 [H,W,3] -> uint8 [H,W]"""
    return ramp_up(plate_distance(frame, plate, radius), lo, hi)


def chroma_key_mask(frame, colour, lo=8, hi=24, rgb=False):
    """keys.ChromaKey(colour, lo, hi) on one frame"""
    kb, kr = key_chroma(colour)
    return mask_from_chroma(frame, kb, kr, *thresholds(kb, kr, lo, hi), rgb=rgb)


# ------------------------------------------------------------------------------------------------ definition
def chroma_def(R, G, B):
    """Exact BT.601 full-range Cb, Cr in float64, round half up, clamp -> (cb, cr) int64"""
    R, G, B = (np.asarray(v).astype(np.float64) for v in (R, G, B))
    Y = KR_ * R + (1.0 - KR_ - KB_) * G + KB_ * B
    cb = np.clip(np.floor((B - Y) / (2.0 * (1.0 - KB_)) + 128.0 + 0.5), 0, 255).astype(np.int64) - 128
    cr = np.clip(np.floor((R - Y) / (2.0 * (1.0 - KR_)) + 128.0 + 0.5), 0, 255).astype(np.int64) - 128
    return cb, cr


def chroma_exact(R, G, B):
    """The same before rounding: (Cb, Cr) float64, for the near-tie analysis"""
    R, G, B = (np.asarray(v).astype(np.float64) for v in (R, G, B))
    Y = KR_ * R + (1.0 - KR_ - KB_) * G + KB_ * B
    return (B - Y) / (2.0 * (1.0 - KB_)) + 128.0, (R - Y) / (2.0 * (1.0 - KR_)) + 128.0


def mask_from_cone_def(cb, cr, kb, kr, qlo, qhi):
    """The cone quantity and the ramp in exact arithmetic (Python integers / fractions: floor of an exact quotient), element by
    element -- on whatever integers cb, cr it is given"""
    from fractions import Fraction
    out = np.empty(np.shape(cb), np.uint8)
    flat_b, flat_r, o = np.ravel(cb), np.ravel(cr), out.reshape(-1)
    for i in range(flat_b.size):
        b, r = int(flat_b[i]), int(flat_r[i])
        q = (b * kb + r * kr) - abs(b * kr - r * kb)
        if q <= qlo:
            o[i] = 255
        elif q >= qhi:
            o[i] = 0
        else:
            o[i] = 255 - math.floor(Fraction((q - qlo) * 255, qhi - qlo))
    return out


def mask_from_plate_def(frame, plate, radius, lo, hi):
    """Brute force: pixel by pixel, neighbour by neighbour with clamped coordinates, the ramp in exact arithmetic"""
    from fractions import Fraction
    f, p = np.asarray(frame).astype(int), np.asarray(plate).astype(int)
    H, W = f.shape[:2]
    out = np.empty((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            d = 255
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    yy, xx = min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)
                    d = min(d, max(abs(int(f[y, x, c]) - int(p[yy, xx, c])) for c in range(3)))
            out[y, x] = 0 if d <= lo else 255 if d >= hi else math.floor(Fraction((d - lo) * 255, hi - lo))
    return out
