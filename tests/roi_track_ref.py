"""Restatement of the tracking window of region-of-interest matting (otvm_amd/roi.py track_origin, csrc/roi.hip otvm_roi_track,
otvm_roi_crop_at, otvm_roi_paste_at) from its definition: the per-axis hold / recentre policy in integers, the crop and the paste at
an origin clamped into the frame, and the windows of a whole clip whose output trimaps are known."""
from tests import roi_ref as R


def empty(box):
    return box[2] < box[0] or box[3] < box[1]


def hold_of(margin):
    return max(1, margin // 2)


def _axis(lo, hi, o, side, full, hold):
    """One axis: the box spans lo .. hi (frame coordinates), the neighbour's window o .. o + side - 1 of 0 .. full - 1."""
    near = lo - o                       # pixels of the window before the box
    far = (o + side - 1) - hi           # and behind it
    near_held = near >= hold or o == 0
    far_held = far >= hold or o + side == full
    if near_held and far_held:
        return o
    centre = (lo + hi + 1) // 2 - side // 2
    return max(0, min(centre, full - side))


def track_origin(box, prev, h, w, H, W, hold):
    """box: the neighbour's non-background box in frame coordinates; prev: its origin, or None = centre on the box."""
    if prev is None:
        if empty(box):
            return (0, 0)
        return (max(0, min((box[0] + box[2] + 1) // 2 - h // 2, H - h)), max(0, min((box[1] + box[3] + 1) // 2 - w // 2, W - w)))
    if empty(box):
        return (prev[0], prev[1])
    return (_axis(box[0], box[2], prev[0], h, H, hold), _axis(box[1], box[3], prev[1], w, W, hold))


def track_row(row, prev, h, w, H, W, hold):
    """What otvm_roi_track writes: ``row`` is otvm_trimap_bbox's eight words, in the neighbour's window when ``prev`` is given
    (clamped into the frame as the kernel clamps what it reads), in the frame otherwise."""
    b = tuple(int(v) for v in row[4:8])
    if prev is None:
        return track_origin(b, None, h, w, H, W, hold)
    py, px = clamp_origin(prev, h, w, H, W)
    return track_origin((b[0] + py, b[1] + px, b[2] + py, b[3] + px) if not empty(b) else b, (py, px), h, w, H, W, hold)


def clamp_origin(origin, h, w, H, W):
    return (max(0, min(int(origin[0]), H - h)), max(0, min(int(origin[1]), W - w)))


def crop_at(origin, size, H, W, frame=None, trimap=None, labels=None):
    return R.crop(clamp_origin(origin, size[0], size[1], H, W) + tuple(size), frame, trimap, labels)


def paste_at(origin, size, H, W, alpha, trimap, fgr=None, frame=None, u8_rgb=False, outside=None):
    return R.paste(clamp_origin(origin, size[0], size[1], H, W) + tuple(size), H, W, alpha, trimap, fgr, frame, u8_rgb, outside)


def neighbour(t, k0):
    """The already-matted temporal neighbour on the side the sweep comes from."""
    return t - 1 if t > k0 else t + 1


def box_inside(window, src):
    """The non-background box of a class map, MEASURED INSIDE the window, in frame coordinates (empty: R's empty box)."""
    y0, x0, h, w = window
    b = R.bbox(R.crop(window, trimap=src)[1] if src.ndim == 3 else R.crop(window, labels=src)[2])[4:]
    b = tuple(int(v) for v in b)
    return b if empty(b) else (b[0] + y0, b[1] + x0, b[2] + y0, b[3] + x0)


def clip_windows(size, H, W, hold, order, key_sources, k0, outputs):
    """The windows of a clip whose steps run in ``order``: a step in ``key_sources`` {t: class map at H x W} centres on its source,
    every other follows ``outputs[neighbour]`` -- the class map the network puts out for that frame where the window shows it
    (background elsewhere) -- measured inside the neighbour's window.  -> ({t: window}, [clipped frames])"""
    h, w = size
    wins, boxes = {}, {}
    for t in order:
        if t in key_sources:
            at = track_origin(tuple(int(v) for v in R.bbox(key_sources[t])[4:]), None, h, w, H, W, hold)
        else:
            n = neighbour(t, k0)
            at = track_origin(boxes[n], wins[n][:2], h, w, H, W, hold)
        wins[t] = at + (h, w)
        boxes[t] = box_inside(wins[t], outputs[t])
    return wins, [t for t in sorted(wins) if touched(wins[t], boxes[t], H, W)]


def touched(window, box, H, W):
    """roi_clipped: the box reaches a side of the window that is not a side of the frame."""
    if empty(box):
        return False
    y0, x0, h, w = window
    return ((box[0] == y0 and y0 > 0) or (box[1] == x0 and x0 > 0) or (box[2] == y0 + h - 1 and y0 + h < H)
            or (box[3] == x0 + w - 1 and x0 + w < W))
