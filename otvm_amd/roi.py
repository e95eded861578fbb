"""Region-of-interest matting, host side: otvm_trimap_bbox, otvm_roi_crop and otvm_roi_paste (include/otvm_hip.h) around device
tensors, and the window policy -- pure host functions, testable without a GPU.  Everything runs on the caller's current stream;
there is no PyTorch fallback.

Checked by definition only: the result of a window is, bit for bit, the matte of the cropped clip pasted back.  It is NOT the
full-frame result (the decoder's pyramid pooling sees the window, not the frame), and the default margin is a PLACEHOLDER: nobody
has tuned it on real footage.

The tracking window (run_video_matte(roi="track")): otvm_roi_track, otvm_roi_crop_at and otvm_roi_paste_at keep the window's origin
on the device, a row of an int32 log per frame; track_origin is the same policy on the host, and rows_of the one read-back."""
import ctypes as C

import numpy as np
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


def hold_of(margin):
    """The pixels a tracked box keeps from a window side before the window moves: max(1, margin // 2).  At least 1: the box is
    measured inside the window, so it can touch a side but never cross it.  (A PLACEHOLDER like the margin itself.)"""
    return max(1, int(margin) // 2)


def track_origin(box, prev, h, w, H, W, hold):
    """(oy, ox) of the h x w tracking window of a frame, from its already-matted temporal neighbour: ``box`` is the non-background
    box of the neighbour's output trimap in FRAME coordinates, ``prev`` the neighbour's origin.  Each axis on its own HOLDS
    ``prev`` while the box keeps at least ``hold`` pixels from both window sides on that axis (a window side that is the frame's
    side always counts as held), and recentres on the box, clamped to the frame, otherwise; an empty box holds both.
    ``prev`` None: a step with a trimap of its own -- window_origin(box), (0, 0) for an empty box.  Pure integer arithmetic;
    otvm_roi_track (csrc/roi.hip) is the same policy on the device, where the box comes in window coordinates."""
    if prev is None:
        return window_origin(box, h, w, H, W)
    if is_empty(box):
        return tuple(prev)
    out = []
    for a, (side, full) in enumerate(((h, H), (w, W))):
        o, lo, hi = prev[a], box[a], box[a + 2]
        held = (lo - o >= hold or o == 0) and (o + side - 1 - hi >= hold or o + side == full)
        out.append(o if held else min(max((lo + hi + 1) // 2 - side // 2, 0), full - side))
    return tuple(out)


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


# ---- roi="track" as run_video_matte and run_video_matte_subjects both take it (``who``: the route, which keeps its messages)
def track_spec(spec, who):
    """'track' -> ("track",), ('track', h, w) -> ("track", h, w) with ints; None for every other form (the caller's own)."""
    if isinstance(spec, str):
        return ("track",) if spec == "track" else None
    if not (isinstance(spec, (tuple, list)) and len(spec) == 3 and spec[0] == "track"):
        return None
    if not all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in spec[1:]) or spec[1] < 1 or spec[2] < 1:
        raise ValueError("%s: roi = ('track', h, w) needs integers h, w >= 1, got %r" % (who, spec))
    return ("track", int(spec[1]), int(spec[2]))


def check_margin(margin, who):
    if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or margin < 0:
        raise ValueError("%s: roi_margin is a number of pixels >= 0 (an integer), got %r" % (who, margin))
    return int(margin)


def check_hold(hold, who="otvm_amd.roi"):
    if isinstance(hold, bool) or int(hold) != hold or hold < 1:
        raise ValueError("%s: hold is a number of pixels >= 1 (an integer), got %r" % (who, hold))
    return int(hold)


def track_size(boxes, spec, margin, H, W, who, what):
    """(h, w) of the ONE size a clip's tracking windows share, from ``boxes`` = {label: non-background box of a source}: window_size
    over all of them for ("track",); ("track", h, w) as given, refused when a box does not fit (``what`` % label names its source)."""
    if len(spec) != 3:
        return window_size(list(boxes.values()), H, W, margin)
    h, w = check_size(spec[1:], H, W, who + ": roi")
    for label, box in sorted(boxes.items()):
        if not is_empty(box) and (box[2] - box[0] + 1 > h or box[3] - box[1] + 1 > w):
            raise ValueError("%s: the %dx%d window of roi = %r does not hold %s (its classes other than background: rows %d ... %d, "
                             "columns %d ... %d)" % (who, h, w, spec, what % label, box[0], box[2], box[1], box[3]))
    return h, w


def new_log(rows_shape, h, w, dev):
    """The int32 [*rows_shape, 10] log of a tracked clip.  Per row: words 0 .. 7 the boxes of the frame's output trimap (in the frame's
    window), words 8, 9 the window's origin -- ONE buffer, read back with one copy after the last frame.  Rows start as the empty
    box at (0, 0)."""
    return torch.tensor([h, w, -1, -1, h, w, -1, -1, 0, 0], dtype=torch.int32, device=dev).repeat(*rows_shape, 1)


def clipped(rows, size, H, W, seen):
    """Read-back rows (eight box words in window coordinates, then the origin) -> (roi: [(y0, x0, h, w) per row], roi_clipped: the
    i of ``seen`` whose non-background box reaches a side of its window that is not a side of the frame)."""
    wins = [(r[8], r[9]) + tuple(size) for r in rows]
    in_frame = lambda r: (r[4] + r[8], r[5] + r[9], r[6] + r[8], r[7] + r[9])                 # (an empty box stays empty)
    return wins, [i for i in sorted(seen) if touched_sides(wins[i], in_frame(rows[i]), H, W)]  # box words of other rows: not looked at


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


def rows_of(buf):
    """A device int32 [n,k] buffer as n host tuples: THE read-back of the tracking window -- the source boxes before the first
    frame, the origin log and the output boxes after the last -- and nothing in between.  (The static window reads its output
    boxes back through it too, once, after the last frame.)"""
    return [tuple(r) for r in buf.cpu().view(buf.shape[0], -1).tolist()]


def check_size(size, H, W, who="otvm_amd.roi"):
    """(h, w) as two ints, refused unless 1 <= h <= H and 1 <= w <= W."""
    try:
        h, w = (int(v) for v in size)
        ok = all(int(v) == v and not isinstance(v, bool) for v in size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: a window size is two integers (h, w), got %r" % (who, size))
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError("%s: the window size (h, w) = %r needs 1 <= h <= %d and 1 <= w <= %d (the %dx%d frame)" % (who, (h, w), H, W, H, W))
    return h, w


def _origin_row(origin, dev, who, words=2):
    if (not torch.is_tensor(origin) or origin.dtype != torch.int32 or origin.numel() != words or not origin.is_contiguous()
            or origin.device != dev):
        raise ValueError("otvm_amd.roi: %s takes %d contiguous int32 on %s" % (who, words, dev))


def track(box, prev, out, size, H, W, hold):
    """otvm_roi_track: ``out`` (row t of the int32 [T,2] origin log) = track_origin of the neighbour's ``box`` row (the int32 [8]
    trimap_bbox wrote, in the neighbour's window) and the neighbour's origin ``prev`` (its row of the log); ``prev`` None: centred
    on ``box``, which is then in frame coordinates (a step with a trimap of its own).  One small launch on the current stream;
    nothing is synchronised."""
    dev = out.device
    _origin_row(box, dev, "track's box", 8)
    _origin_row(out, dev, "track's out")
    if prev is not None:
        _origin_row(prev, dev, "track's prev")
    h, w = check_size(size, H, W)
    p = L.RoiTrackParams()
    p.box, p.prev, p.out = box.data_ptr(), None if prev is None else prev.data_ptr(), out.data_ptr()
    p.H, p.W, p.h, p.w, p.hold = H, W, h, w, check_hold(hold)
    L.check(L.load().otvm_roi_track(C.byref(p), _stream(dev)), "roi_track")
    return out


def boxes_of(rows):
    """A read-back [T,8] buffer (or one row) as host tuples: ([unknown box per row], [non-bg box per row])."""
    rows = rows.cpu().view(-1, 8).tolist()
    return [tuple(r[:4]) for r in rows], [tuple(r[4:]) for r in rows]


def crop(window, frame=None, trimap=None, labels=None, origin=None):
    """The window (y0, x0, h, w) of whichever of frame uint8 [H,W,3], trimap float [3,H,W] and labels uint8 [H,W] are given, in
    ONE launch: (frame, trimap, labels) with None where nothing was given.  (``origin``: crop_at's, ``window`` then being (h, w).)"""
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
    if origin is None:
        y0, x0, h, w = check_window(window, H, W)
    else:
        (y0, x0), (h, w) = (0, 0), check_size(window, H, W)
        _origin_row(origin, dev, "crop_at")
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
    if origin is None:
        L.check(L.load().otvm_roi_crop(C.byref(p), _stream(dev)), "roi_crop")
    else:
        L.check(L.load().otvm_roi_crop_at(C.byref(p), origin.data_ptr(), _stream(dev)), "roi_crop_at")
    return tuple(out)


def crop_at(origin, size, frame=None, trimap=None, labels=None):
    """crop() of the (h, w) = ``size`` window whose origin the KERNEL reads from ``origin``, two int32 on the device (a row of the
    [T,2] log track() writes) -- clamped there to [0, H - h] x [0, W - w] whatever the row holds.  Nothing is synchronised."""
    return crop(size, frame, trimap, labels, origin=origin)


def paste(window, H, W, alpha, trimap, fgr=None, frame=None, rgb=False, outside=None, want=("alpha", "alpha_u8", "trimap", "fgr"),
          origin=None):
    """A window's results back at H x W in one pass.  alpha [h,w], trimap [3,h,w], fgr [3,h,w] (R, G, B; optional) are the
    window's; ``frame`` uint8 [H,W,3] gives F outside the window, ``outside`` (one-hot [3,H,W] or None = background) the trimap
    and alpha there.  Returns (alpha [H,W], alpha_u8 [H,W], trimap [3,H,W], fgr [3,H,W]), None for what ``want`` leaves out or
    (fgr) what has no source.  (``origin``: paste_at's, ``window`` then being (h, w).)"""
    dev = alpha.device
    if origin is None:
        y0, x0, h, w = check_window(window, H, W)
    else:
        (y0, x0), (h, w) = (0, 0), check_size(window, H, W)
        _origin_row(origin, dev, "paste_at")
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
    if origin is None:
        L.check(L.load().otvm_roi_paste(C.byref(p), _stream(dev)), "roi_paste")
    else:
        L.check(L.load().otvm_roi_paste_at(C.byref(p), origin.data_ptr(), _stream(dev)), "roi_paste_at")
    return res.get("alpha"), res.get("alpha_u8"), res.get("trimap"), res.get("fgr")


def paste_at(origin, size, H, W, alpha, trimap, fgr=None, frame=None, rgb=False, outside=None, want=("alpha", "alpha_u8", "trimap", "fgr")):
    """paste() of the (h, w) = ``size`` window whose origin the KERNEL reads from ``origin`` (as crop_at)."""
    return paste(size, H, W, alpha, trimap, fgr, frame, rgb, outside, want, origin=origin)
