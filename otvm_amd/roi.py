"""Region-of-interest matting, host side: otvm_trimap_bbox, otvm_roi_crop and otvm_roi_paste (include/otvm_hip.h) around device
tensors, and the window policy -- pure host functions, testable without a GPU.  Everything runs on the caller's current stream;
there is no PyTorch fallback.

Checked by definition only: the result of a window is, bit for bit, the matte of the cropped clip pasted back.  It is NOT the
full-frame result (the decoder's pyramid pooling sees the window, not the frame), and the default margin is a PLACEHOLDER: nobody
has tuned it on real footage."""
import ctypes as C

import torch

from . import lib as L

ALIGN = 32             # the engine pads to multiples of 32 (engine.pad_amounts(..., 32)): a window that is one pads nothing


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------ the window policy (host only)
def is_empty(box):
    """A box is (y0, x0, y1, x1), inclusive; the kernel's empty box is (H, W, -1, -1)."""
    return box[2] < box[0] or box[3] < box[1]


def union(boxes):
    """The smallest box round the non-empty ones, or None when there is none."""
    live = [b for b in boxes if not is_empty(b)]
    if not live:
        return None
    return (min(b[0] for b in live), min(b[1] for b in live), max(b[2] for b in live), max(b[3] for b in live))


def _side(need, full):
    s = ALIGN * ((need + ALIGN - 1) // ALIGN)
    return full if s > full else s


def window_size(boxes, H, W, margin):
    """(h, w) of ONE window that holds any of ``boxes`` with ``margin`` pixels round it: the largest extent plus twice the margin,
    rounded up to a multiple of ALIGN, the frame's side where that exceeds it.  No non-empty box: (min(H, 32), min(W, 32))."""
    live = [b for b in boxes if not is_empty(b)]
    if not live:
        return min(H, ALIGN), min(W, ALIGN)
    need_h = max(b[2] - b[0] + 1 for b in live) + 2 * margin
    need_w = max(b[3] - b[1] + 1 for b in live) + 2 * margin
    return _side(need_h, H), _side(need_w, W)


def window_origin(box, h, w, H, W, previous=(0, 0)):
    """(oy, ox) of the h x w window centred on ``box`` and clamped to the frame; an empty box keeps ``previous``."""
    if is_empty(box):
        return tuple(previous)
    oy = min(max((box[0] + box[2] + 1) // 2 - h // 2, 0), H - h)
    ox = min(max((box[1] + box[3] + 1) // 2 - w // 2, 0), W - w)
    return oy, ox


def contains(window, box):
    """Does the window (y0, x0, h, w) hold every pixel of ``box``?  (An empty box lies in every window.)"""
    if is_empty(box):
        return True
    y0, x0, h, w = window
    return y0 <= box[0] and x0 <= box[1] and box[2] < y0 + h and box[3] < x0 + w


def touched_sides(window, box, H, W):
    """Does ``box`` reach a side of the window that is not a side of the frame?  (What roi_clipped lists.)"""
    if is_empty(box):
        return False
    y0, x0, h, w = window
    return ((box[0] <= y0 and y0 > 0) or (box[1] <= x0 and x0 > 0) or (box[2] >= y0 + h - 1 and y0 + h < H)
            or (box[3] >= x0 + w - 1 and x0 + w < W))


def check_window(window, H, W, who="otvm_amd.roi"):
    """(y0, x0, h, w) as four ints, refused when it is empty or leaves the H x W frame."""
    try:
        y0, x0, h, w = (int(v) for v in window)
        ok = all(int(v) == v and not isinstance(v, bool) for v in window)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: a window is four integers (y0, x0, h, w), got %r" % (who, window))
    if h < 1 or w < 1:
        raise ValueError("%s: the window (y0, x0, h, w) = %r is empty" % (who, (y0, x0, h, w)))
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError("%s: the window (y0, x0, h, w) = %r leaves the %dx%d frame" % (who, (y0, x0, h, w), H, W))
    return y0, x0, h, w


# ------------------------------------------------------------------ the kernels round device tensors
def _source(src, who):
    """A class map as the kernels take it: ('trimap', float [3,H,W]) or ('labels', uint8 [H,W]), contiguous, on the GPU."""
    if not torch.is_tensor(src) or not src.is_cuda:
        raise ValueError("otvm_amd.roi: %s takes a tensor on the GPU" % who)
    if src.dim() == 3 and src.shape[0] == 3 and src.dtype == torch.float32:
        return "trimap", src.contiguous()
    if src.dim() == 2 and src.dtype == torch.uint8:
        return "labels", src.contiguous()
    raise ValueError("otvm_amd.roi: %s takes a float32 trimap [3,H,W] or a uint8 label map [H,W], got %s %s"
                     % (who, src.dtype, tuple(src.shape)))


def trimap_bbox(src, out=None):
    """The boxes of a float trimap [3,H,W] or a uint8 label map [H,W] on the device: int32 [8] = y0, x0, y1, x1 (inclusive) of the
    unknown pixels, then of the non-background pixels; an empty set is (H, W, -1, -1).  ``out``: an int32 [8] view to write into
    (slot t of a [T,8] buffer: a clip is read back with one copy); a fresh tensor otherwise.  Nothing is synchronised."""
    kind, src = _source(src, "trimap_bbox")
    if out is None:
        out = torch.empty(8, dtype=torch.int32, device=src.device)
    elif out.dtype != torch.int32 or out.numel() != 8 or not out.is_contiguous() or out.device != src.device:
        raise ValueError("otvm_amd.roi: trimap_bbox writes 8 contiguous int32 on %s" % src.device)
    p = L.RoiBboxParams()
    setattr(p, kind, src.data_ptr())
    p.H, p.W, p.out = src.shape[-2], src.shape[-1], out.data_ptr()
    L.check(L.load().otvm_trimap_bbox(C.byref(p), _stream(src.device)), "trimap_bbox")
    return out


def boxes_of(rows):
    """A read-back [T,8] buffer (or one row) as host tuples: ([unknown box per row], [non-bg box per row])."""
    rows = rows.cpu().view(-1, 8).tolist()
    return [tuple(r[:4]) for r in rows], [tuple(r[4:]) for r in rows]


def crop(window, frame=None, trimap=None, labels=None):
    """The window (y0, x0, h, w) of whichever of frame uint8 [H,W,3], trimap float [3,H,W] and labels uint8 [H,W] are given, in
    ONE launch: (frame, trimap, labels) with None where nothing was given."""
    given = [x for x in (frame, trimap, labels) if x is not None]
    if not given:
        raise ValueError("otvm_amd.roi: crop needs a frame, a trimap or a label map")
    dev = given[0].device
    if frame is not None and (frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3):
        raise ValueError("otvm_amd.roi: a frame is uint8 [H,W,3], got %s %s" % (frame.dtype, tuple(frame.shape)))
    if trimap is not None and (trimap.dtype != torch.float32 or trimap.dim() != 3 or trimap.shape[0] != 3):
        raise ValueError("otvm_amd.roi: a trimap is float32 [3,H,W], got %s %s" % (trimap.dtype, tuple(trimap.shape)))
    if labels is not None and (labels.dtype != torch.uint8 or labels.dim() != 2):
        raise ValueError("otvm_amd.roi: a label map is uint8 [H,W], got %s %s" % (labels.dtype, tuple(labels.shape)))
    sizes = {tuple(x.shape[:2]) if x is frame else tuple(x.shape[-2:]) for x in given}
    if len(sizes) != 1 or any(not x.is_cuda or x.device != dev for x in given):
        raise ValueError("otvm_amd.roi: crop takes tensors of one resolution on one GPU, got %s" % sorted(sizes))
    (H, W), = sizes
    y0, x0, h, w = check_window(window, H, W)
    p = L.RoiCropParams()
    p.H, p.W, p.y0, p.x0, p.h, p.w = H, W, y0, x0, h, w
    out = [None, None, None]
    keep = []
    for j, (name, x, shape) in enumerate((("frame", frame, (h, w, 3)), ("trimap", trimap, (3, h, w)), ("labels", labels, (h, w)))):
        if x is not None:
            x = x.contiguous()
            keep.append(x)
            out[j] = torch.empty(shape, dtype=x.dtype, device=dev)
            setattr(p, name, x.data_ptr())
            setattr(p, name + "_out", out[j].data_ptr())
    L.check(L.load().otvm_roi_crop(C.byref(p), _stream(dev)), "roi_crop")
    return tuple(out)


def paste(window, H, W, alpha, trimap, fgr=None, frame=None, rgb=False, outside=None, want=("alpha", "alpha_u8", "trimap", "fgr")):
    """A window's results back at H x W in one pass.  alpha [h,w], trimap [3,h,w], fgr [3,h,w] (R, G, B; optional) are the
    window's; ``frame`` uint8 [H,W,3] gives F outside the window, ``outside`` (one-hot [3,H,W] or None = background) the trimap
    and alpha there.  Returns (alpha [H,W], alpha_u8 [H,W], trimap [3,H,W], fgr [3,H,W]), None for what ``want`` leaves out or
    (fgr) what has no source."""
    dev = alpha.device
    y0, x0, h, w = check_window(window, H, W)
    alpha, trimap = alpha.contiguous(), trimap.contiguous()
    if tuple(alpha.shape) != (h, w) or tuple(trimap.shape) != (3, h, w) or alpha.dtype != torch.float32 or trimap.dtype != torch.float32:
        raise ValueError("otvm_amd.roi: paste takes the window's fp32 alpha [%d,%d] and trimap [3,%d,%d], got %s and %s"
                         % (h, w, h, w, tuple(alpha.shape), tuple(trimap.shape)))
    p = L.RoiPasteParams()
    p.H, p.W, p.y0, p.x0, p.h, p.w, p.u8_rgb = H, W, y0, x0, h, w, int(bool(rgb))
    p.win_alpha, p.win_trimap = alpha.data_ptr(), trimap.data_ptr()
    keep = [alpha, trimap]
    with_fgr = "fgr" in want and fgr is not None
    if with_fgr:
        fgr = fgr.contiguous()
        if frame is None or tuple(fgr.shape) != (3, h, w) or fgr.dtype != torch.float32:
            raise ValueError("otvm_amd.roi: the pasted F needs the window's fp32 F [3,%d,%d] and the frame" % (h, w))
        frame = frame.contiguous()
        if tuple(frame.shape) != (H, W, 3) or frame.dtype != torch.uint8:
            raise ValueError("otvm_amd.roi: the frame is uint8 [%d,%d,3], got %s %s" % (H, W, frame.dtype, tuple(frame.shape)))
        p.win_fgr, p.frame = fgr.data_ptr(), frame.data_ptr()
        keep += [fgr, frame]
    if outside is not None:
        outside = outside.contiguous()
        if tuple(outside.shape) != (3, H, W) or outside.dtype != torch.float32:
            raise ValueError("otvm_amd.roi: `outside` is a one-hot fp32 trimap [3,%d,%d], got %s" % (H, W, tuple(outside.shape)))
        p.outside = outside.data_ptr()
        keep.append(outside)
    res = {}
    for name, shape, dt in (("alpha", (H, W), torch.float32), ("alpha_u8", (H, W), torch.uint8), ("trimap", (3, H, W), torch.float32),
                            ("fgr", (3, H, W), torch.float32)):
        if name in want and (name != "fgr" or with_fgr):
            res[name] = torch.empty(shape, dtype=dt, device=dev)
            setattr(p, name, res[name].data_ptr())
    L.check(L.load().otvm_roi_paste(C.byref(p), _stream(dev)), "roi_paste")
    return res.get("alpha"), res.get("alpha_u8"), res.get("trimap"), res.get("fgr")
