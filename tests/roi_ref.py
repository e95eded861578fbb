"""numpy restatement of the region-of-interest kernels (include/otvm_hip.h: otvm_trimap_bbox, otvm_roi_crop, otvm_roi_paste),
operation by operation, a brute-force box (plain loops over pixels) the restated box is held against, and the window policy of
otvm_amd/roi.py written out again from its definition."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------ otvm_trimap_bbox
def class_masks(src):
    """(unknown, non-background) boolean [H,W] of a float trimap [3,H,W] or a uint8 label map [H,W]."""
    src = np.asarray(src)
    if src.ndim == 3:
        t0, t1, t2 = (np.asarray(src[k], F32) for k in range(3))
        with np.errstate(invalid="ignore"):
            nonbg = (t1 > t0) | (t2 > t0)                  # max(t1, t2) > t0
            unknown = nonbg & (t1 >= t2)
        return unknown, nonbg
    assert src.dtype == np.uint8 and src.ndim == 2
    return src == 1, (src == 1) | (src == 2)


def _box(m):
    H, W = m.shape
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    if rows.size == 0:
        return (H, W, -1, -1)
    return (int(rows[0]), int(cols[0]), int(rows[-1]), int(cols[-1]))


def bbox(src):
    """int32 [8]: y0, x0, y1, x1 (inclusive) of the unknown pixels, then of the non-background pixels; empty = (H, W, -1, -1)."""
    unknown, nonbg = class_masks(src)
    return np.array(_box(unknown) + _box(nonbg), np.int32)


def bbox_brute(src):
    """The same by plain loops over the pixels, from the definition."""
    src = np.asarray(src)
    H, W = src.shape[-2:]
    out = [H, W, -1, -1, H, W, -1, -1]
    for y in range(H):
        for x in range(W):
            if src.ndim == 3:
                t0, t1, t2 = float(src[0, y, x]), float(src[1, y, x]), float(src[2, y, x])
                nonbg = max(t1, t2) > t0
                unknown = nonbg and t1 >= t2
            else:
                v = int(src[y, x])
                unknown, nonbg = v == 1, v in (1, 2)
            for s, hit in ((0, unknown), (4, nonbg)):
                if hit:
                    out[s], out[s + 1] = min(out[s], y), min(out[s + 1], x)
                    out[s + 2], out[s + 3] = max(out[s + 2], y), max(out[s + 3], x)
    return np.array(out, np.int32)


# ------------------------------------------------------------------ otvm_roi_crop
def crop(window, frame=None, trimap=None, labels=None):
    y0, x0, h, w = window
    return (None if frame is None else np.ascontiguousarray(np.asarray(frame)[y0:y0 + h, x0:x0 + w]),
            None if trimap is None else np.ascontiguousarray(np.asarray(trimap)[:, y0:y0 + h, x0:x0 + w]),
            None if labels is None else np.ascontiguousarray(np.asarray(labels)[y0:y0 + h, x0:x0 + w]))


# ------------------------------------------------------------------ otvm_roi_paste
def quant_u8(a):
    """(uint8) min(max(trunc(a * 255.f), 0), 255); a non-finite alpha gives 0."""
    a = np.asarray(a, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.minimum(np.maximum(np.trunc(a * F32(255.0)), F32(0.0)), F32(255.0))
    return np.where(np.isfinite(a), t, F32(0.0)).astype(np.uint8)


def paste(window, H, W, alpha, trimap, fgr=None, frame=None, u8_rgb=False, outside=None):
    """-> (alpha [H,W], alpha_u8 [H,W], trimap [3,H,W], fgr [3,H,W] or None without the window's F)."""
    y0, x0, h, w = window
    tri = np.zeros((3, H, W), F32)
    if outside is None:
        tri[0] = F32(1.0)
    else:
        tri[:] = np.asarray(outside, F32)
    a = np.where(tri[2] == F32(1.0), F32(1.0), F32(0.0)).astype(F32)
    a[y0:y0 + h, x0:x0 + w] = np.asarray(alpha, F32)
    tri[:, y0:y0 + h, x0:x0 + w] = np.asarray(trimap, F32)
    F = None
    if fgr is not None:
        order = (0, 1, 2) if u8_rgb else (2, 1, 0)
        s = F32(1.0) / F32(255.0)
        F = np.stack([np.asarray(frame)[..., order[c]].astype(F32) * s for c in range(3)]).astype(F32)
        F[:, y0:y0 + h, x0:x0 + w] = np.asarray(fgr, F32)
    return a, quant_u8(a), tri, F


# ------------------------------------------------------------------ the window policy, from its definition
def _ceil32(n):
    return -(-n // 32) * 32


def window_size(boxes, H, W, margin):
    live = [b for b in boxes if b[2] >= b[0] and b[3] >= b[1]]
    if not live:
        return min(H, 32), min(W, 32)
    h = _ceil32(max(b[2] - b[0] + 1 for b in live) + 2 * margin)
    w = _ceil32(max(b[3] - b[1] + 1 for b in live) + 2 * margin)
    return (H if h > H else h), (W if w > W else w)


def window_origin(box, h, w, H, W, previous=(0, 0)):
    if box[2] < box[0] or box[3] < box[1]:
        return tuple(previous)
    return (int(np.clip((box[0] + box[2] + 1) // 2 - h // 2, 0, H - h)), int(np.clip((box[1] + box[3] + 1) // 2 - w // 2, 0, W - w)))


def tracking_windows(unknown_boxes, H, W, margin):
    """roi="auto" with masks=: one size for the clip, an origin per frame."""
    h, w = window_size(unknown_boxes, H, W, margin)
    out, at = [], (0, 0)
    for b in unknown_boxes:
        at = window_origin(b, h, w, H, W, at)
        out.append(at + (h, w))
    return out


def static_window(nonbg_boxes, H, W, margin):
    """roi="auto" with trimap= / mask= / keyframes=: one window round the union of the sources' non-background boxes."""
    live = [b for b in nonbg_boxes if b[2] >= b[0] and b[3] >= b[1]]
    if not live:
        return (0, 0, min(H, 32), min(W, 32))
    u = (min(b[0] for b in live), min(b[1] for b in live), max(b[2] for b in live), max(b[3] for b in live))
    h, w = window_size([u], H, W, margin)
    return window_origin(u, h, w, H, W) + (h, w)
