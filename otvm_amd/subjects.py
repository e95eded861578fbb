"""Multi-subject matting: one clip, S subjects, a matte per subject.  Every subject is followed by a tracking window of its own
(otvm_amd/roi.py, roi="track"); the S windows share ONE size, differ only in their origins -- which live on the device -- and go
through the network as one lock-step batch (EvalModel.forward_batch: one launch per layer over the S windows, one memory bank per
subject).  otvm_subjects_track, otvm_subjects_crop, otvm_subjects_bbox and otvm_subjects_resolve (include/otvm_hip.h) are the glue:
the tracking window's launches over all S subjects at once, and one sweep over the frame that pastes the S windows and settles the
pixels where they overlap.  Everything runs on the caller's current stream; there is no PyTorch fallback.

Checked BY DEFINITION ONLY, with synthetic weights: each subject's matte is, bit for bit (under equal kernel configurations), what
run_video_matte(trimap=that subject, roi=("track", h, w)) gives for it alone, and union / owner / the normalised mattes are the
restatement in tests/subjects_ref.py of those.  Nothing is said about matting quality -- there is no trained checkpoint -- and the
rule of overlap="normalise" and the default margin are untuned PLACEHOLDERS."""
import ctypes as C

import numpy as np
import torch

from . import guided
from . import lib as L
from . import roi as _roi
from .masks import Mask
from .video import _as_tensor, _foreground_option, _ones_alpha, memory_schedule

MAX = L.SUBJECTS_MAX
WHO = "run_video_matte_subjects"
OUTPUTS = ("alpha", "alpha_u8", "trimap", "fgr", "union", "union_u8", "owner")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def rows_of(buf):
    """A device int32 buffer as nested host lists: THE read-back of the route -- the subjects' boxes before the first frame, the
    log after the last -- and nothing in between."""
    return buf.cpu().tolist()


# ------------------------------------------------------------------ the shared window (host only)
def shared_size(boxes, spec, margin, H, W):
    """(h, w) of the ONE window size all subjects share: roi.track_size over the non-background boxes of their first-frame trimaps"""
    return _roi.track_size(dict(enumerate(boxes)), spec, margin, H, W, WHO, "the trimap of subject %d")


def check_roi(spec, margin):
    """-> (None | ("track",) | ("track", h, w), margin): the forms run_video_matte_subjects takes, refused host-side otherwise."""
    margin = _roi.check_margin(margin, WHO)
    track = _roi.track_spec(spec, WHO)
    if spec is not None and track is None:
        raise ValueError("%s: roi is None, 'track' or ('track', h, w): every subject is followed by a window of its own, all of one "
                         "size ('auto' and a static window (y0, x0, h, w) belong to run_video_matte), got %r" % (WHO, spec))
    return track, margin


# ------------------------------------------------------------------ the kernels round device tensors
def _rows(t, S, words, dev, what):
    """(base pointer, stride in words) of S rows of ``words`` int32 on the device: a [S,words] view whose rows are contiguous (a
    slice of the [S,T,10] log)."""
    if (not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or tuple(t.shape) != (S, words) or t.device != dev
            or (words > 1 and t.stride(1) != 1)):
        raise ValueError("otvm_amd.subjects: %s takes int32 [%d,%d] on %s with contiguous rows" % (what, S, words, dev))
    return t.data_ptr(), int(t.stride(0))


def _count(S):
    if isinstance(S, bool) or not 1 <= S <= MAX:
        raise ValueError("otvm_amd.subjects: 1 .. %d subjects, got %d" % (MAX, S))
    return S


def _planes(xs, shape, what):
    xs = [x.contiguous() for x in xs]
    for x in xs:
        if x.dtype != torch.float32 or tuple(x.shape) != shape:
            raise ValueError("otvm_amd.subjects: %s is fp32 %s per subject, got %s %s" % (what, list(shape), x.dtype, tuple(x.shape)))
    return xs


def track(box, prev, out, size, H, W, hold):
    """otvm_subjects_track: roi.track for S subjects in one launch.  ``box`` int32 [S,8] (the rows trimap_bbox wrote for the
    neighbouring frame), ``prev`` int32 [S,2] (the neighbour's origins) or None (every subject centres on its box, then in frame
    coordinates), ``out`` int32 [S,2]; each a view with contiguous rows (slices of the [S,T,10] log).  Nothing is synchronised."""
    S, dev = _count(out.shape[0]), out.device
    p = L.SubjectsTrackParams()
    p.S = S
    p.box_base, p.box_stride = _rows(box, S, 8, dev, "track's box")
    p.out_base, p.out_stride = _rows(out, S, 2, dev, "track's out")
    if prev is not None:
        p.prev_base, p.prev_stride = _rows(prev, S, 2, dev, "track's prev")
    h, w = _roi.check_size(size, H, W, "otvm_amd.subjects")
    p.H, p.W, p.h, p.w, p.hold = H, W, h, w, _roi.check_hold(hold, "otvm_amd.subjects")
    L.check(L.load().otvm_subjects_track(C.byref(p), _stream(dev)), "subjects_track")
    return out


def crop(origins, size, frame=None, trimaps=None):
    """otvm_subjects_crop: the (h, w) = ``size`` windows at the S ``origins`` (int32 [S,2] on the device, clamped by the kernel) of
    the frame uint8 [H,W,3] and / or of S trimaps fp32 [3,H,W], in ONE launch: ([S frame windows] or None, [S trimap windows] or
    None).  Nothing is synchronised."""
    if frame is None and trimaps is None:
        raise ValueError("otvm_amd.subjects: crop needs the frame or the trimaps")
    S, dev = _count(origins.shape[0]), origins.device
    p = L.SubjectsCropParams()
    if frame is not None:
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3 or frame.device != dev:
            raise ValueError("otvm_amd.subjects: a frame is uint8 [H,W,3] on %s, got %s %s" % (dev, frame.dtype, tuple(frame.shape)))
        frame = frame.contiguous()
        H, W = frame.shape[:2]
    if trimaps is not None:
        if len(trimaps) != S:
            raise ValueError("otvm_amd.subjects: crop takes one trimap per subject, got %d for %d" % (len(trimaps), S))
        H, W = (H, W) if frame is not None else tuple(trimaps[0].shape[-2:])
        trimaps = _planes(trimaps, (3, H, W), "a trimap [3,H,W]")
    h, w = _roi.check_size(size, H, W, "otvm_amd.subjects")
    p.S, p.H, p.W, p.h, p.w = S, H, W, h, w
    p.origin_base, p.origin_stride = _rows(origins, S, 2, dev, "crop's origins")
    fo = to = None
    if frame is not None:
        p.frame = frame.data_ptr()
        fo = torch.empty((S, h, w, 3), dtype=torch.uint8, device=dev)
        for s in range(S):
            p.frame_out[s] = fo[s].data_ptr()
    if trimaps is not None:
        to = torch.empty((S, 3, h, w), dtype=torch.float32, device=dev)
        for s in range(S):
            p.trimap[s], p.trimap_out[s] = trimaps[s].data_ptr(), to[s].data_ptr()
    L.check(L.load().otvm_subjects_crop(C.byref(p), _stream(dev)), "subjects_crop")
    return (None if fo is None else list(fo.unbind(0))), (None if to is None else list(to.unbind(0)))


def bbox(trimaps, out):
    """otvm_subjects_bbox: roi.trimap_bbox of S fp32 trimaps [3,h,w] into the S rows of ``out`` (int32 [S,8], a view with contiguous
    rows): two launches whatever S is.  Nothing is synchronised."""
    S, dev = _count(len(trimaps)), out.device
    h, w = trimaps[0].shape[-2:]
    trimaps = _planes(trimaps, (3, h, w), "a trimap [3,h,w]")
    p = L.SubjectsBboxParams()
    p.S, p.H, p.W = S, h, w
    for s in range(S):
        p.trimap[s] = trimaps[s].data_ptr()
    p.out_base, p.out_stride = _rows(out, S, 8, dev, "bbox's out")
    L.check(L.load().otvm_subjects_bbox(C.byref(p), _stream(dev)), "subjects_bbox")
    return out


def resolve(origins, size, H, W, alphas, trimaps, fgrs=None, frame=None, rgb=False, normalise=False,
            want=("alpha", "alpha_u8", "trimap", "union", "union_u8", "owner")):
    """otvm_subjects_resolve: the S windows' results at H x W in one sweep.  ``alphas`` S x [h,w], ``trimaps`` S x [3,h,w], ``fgrs``
    S x [3,h,w] (R, G, B; with "fgr" in ``want``, which also needs the ``frame`` uint8 [H,W,3]); ``origins`` int32 [S,2] on the
    device.  Returns a dict of what ``want`` names: alpha [S,H,W], alpha_u8 [S,H,W], trimap [S,3,H,W], fgr [S,3,H,W], union [H,W],
    union_u8 [H,W], owner [H,W] (uint8: the subject a pixel belongs to, 255 = none).  Nothing is synchronised."""
    S, dev = _count(len(alphas)), origins.device
    h, w = _roi.check_size(size, H, W, "otvm_amd.subjects")
    unknown = [n for n in want if n not in OUTPUTS]
    if unknown or not want:
        raise ValueError("otvm_amd.subjects: resolve's outputs are %s (at least one), got %r" % (", ".join(OUTPUTS), tuple(want)))
    if len(trimaps) != S:
        raise ValueError("otvm_amd.subjects: resolve takes one trimap per subject, got %d for %d" % (len(trimaps), S))
    alphas, trimaps = _planes(alphas, (h, w), "a window alpha [h,w]"), _planes(trimaps, (3, h, w), "a window trimap [3,h,w]")
    p = L.SubjectsResolveParams()
    p.S, p.H, p.W, p.h, p.w, p.u8_rgb, p.normalise = S, H, W, h, w, int(bool(rgb)), int(bool(normalise))
    p.origin_base, p.origin_stride = _rows(origins, S, 2, dev, "resolve's origins")
    for s in range(S):
        p.win_alpha[s], p.win_trimap[s] = alphas[s].data_ptr(), trimaps[s].data_ptr()
    if "fgr" in want:
        if fgrs is None or frame is None or len(fgrs) != S:
            raise ValueError("otvm_amd.subjects: the resolved F needs every subject's fp32 F [3,%d,%d] and the frame" % (h, w))
        fgrs, frame = _planes(fgrs, (3, h, w), "a window F [3,h,w]"), frame.contiguous()
        if tuple(frame.shape) != (H, W, 3) or frame.dtype != torch.uint8:
            raise ValueError("otvm_amd.subjects: the frame is uint8 [%d,%d,3], got %s %s" % (H, W, frame.dtype, tuple(frame.shape)))
        p.frame = frame.data_ptr()
        for s in range(S):
            p.win_fgr[s] = fgrs[s].data_ptr()
    res = {}
    for name, field, shape, dt in (("alpha", "alpha", (S, H, W), torch.float32), ("alpha_u8", "alpha_u8", (S, H, W), torch.uint8),
                                   ("trimap", "trimap", (S, 3, H, W), torch.float32), ("fgr", "fgr", (S, 3, H, W), torch.float32),
                                   ("union", "union_alpha", (H, W), torch.float32), ("union_u8", "union_u8", (H, W), torch.uint8),
                                   ("owner", "owner", (H, W), torch.uint8)):
        if name in want:
            res[name] = torch.empty(shape, dtype=dt, device=dev)
            setattr(p, field, res[name].data_ptr())
    L.check(L.load().otvm_subjects_resolve(C.byref(p), _stream(dev)), "subjects_resolve")
    return res


# ------------------------------------------------------------------ the route
def _refuse(model, frames, subjects, roi, roi_margin, overlap):
    """Every refusal that needs no device, before anything is uploaded -> (roi spec, margin)."""
    from . import engine
    spec, margin = check_roi(roi, roi_margin)
    if overlap not in ("keep", "normalise"):
        raise ValueError("%s: overlap is 'keep' or 'normalise', got %r" % (WHO, overlap))
    if not isinstance(subjects, (list, tuple)) or not 1 <= len(subjects) <= MAX:
        raise ValueError("%s: `subjects` is a list of 1 .. %d first-frame trimaps [3,H,W] or Masks, one per subject, got %s"
                         % (WHO, MAX, "%d" % len(subjects) if isinstance(subjects, (list, tuple)) else type(subjects).__name__))
    core = model.module if hasattr(model, "module") else model
    name = getattr(core, "precision", None) or engine.default_precision()
    if name != "f16x3":
        raise ValueError("%s: the subjects run as one lock-step batch, which the engine has on the f16x3 path only (and which is "
                         "checked there only); the model's precision is %r" % (WHO, name))
    sizes = []
    for s, v in enumerate(subjects):
        if isinstance(v, Mask):
            if v.role != "key":
                raise ValueError("%s: subject %d is a Mask with role %r; a subject is its first-frame trimap: role 'key'" % (WHO, s, v.role))
            v.band_for(model)                                 # (a missing band is refused before anything is uploaded)
            sizes.append(tuple(v.shape))
        else:
            shape = tuple(np.shape(v))
            if len(shape) != 3 or shape[0] != 3:
                raise ValueError("%s: subject %d is a one-hot trimap [3,H,W] or a Mask, got shape %s" % (WHO, s, shape))
            sizes.append(shape[1:])
    if len(set(sizes)) != 1:
        raise ValueError("%s: the subjects are given at the frames' resolution, all of them; got %s" % (WHO, sorted(set(sizes))))
    if len(frames) > 0 and (isinstance(frames, (list, tuple, np.ndarray)) or torch.is_tensor(frames)):
        _check_frame(_as_tensor(frames[0]), 0, sizes[0])
    return spec, margin, sizes[0]


def _check_frame(f, t, HW):
    if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
        raise ValueError("%s: takes uint8 [H,W,3] frames (float frames have no window route), got %s %s" % (WHO, f.dtype, tuple(f.shape)))
    if tuple(f.shape[:2]) != tuple(HW):
        raise ValueError("%s: frame %d is %dx%d, the subjects are %dx%d (subjects are given at the frames' resolution)"
                         % ((WHO, t) + tuple(f.shape[:2]) + tuple(HW)))


@torch.no_grad()
def run_video_matte_subjects(model, frames, subjects, roi="track", roi_margin=32, overlap="keep", skip=10, max_num=5,
                             frames_are_rgb=False, foreground=False, keep_on_device=False, on_frame=None, device=None, key=None):
    """Matte S subjects of ONE clip in one pass: a full-resolution matte per subject, their union and an owner map.

    model      : EvalModel on the GPU, precision f16x3 (the lock-step batch's own limit)
    frames     : uint8 [H,W,3] images, BGR unless frames_are_rgb
    subjects   : 1 .. 8 entries, each the subject's first-frame trimap -- one-hot [3,H,W] or a masks.Mask (role "key", converted
                 once at H x W)
    roi        : "track": every subject is followed by a tracking window of its own (run_video_matte's roi="track": the origin
                 lives on the device, follows the non-background box of the trimap returned for the previous frame and LAGS ONE
                 FRAME), all of ONE size -- roi.window_size over every subject's non-background box plus ``roi_margin``, rounded up
                 to 32; the boxes are read back once, before the first frame.  ("track", h, w): the size as given, refused when a
                 subject's box does not fit.  None: the window is the frame (no crop, no tracking; S full-frame sequences in
                 lock-step).  The S windows go through the network as one batch (EvalModel.forward_batch: a memory bank per
                 subject, the memory schedule -- large-input rule included -- evaluated at h x w).
    overlap    : what a pixel gets where windows overlap.  "keep": every subject's alpha as its window gave it -- each subject's
                 planes are then exactly run_video_matte(trimap=that subject, roi=("track", h, w)).  "normalise": where the alphas
                 of a pixel sum above 1 each is divided by the sum (an untuned PLACEHOLDER, like the margin).  ``union`` is
                 min(sum, 1) of the alphas as the windows gave them either way; outside its window a subject is background.
    foreground : also "fgr_u8" [S,T,H,W,4]: per subject the network's F inside its window, the frame outside, A = alpha_u8
    on_frame   : callable(t, alpha [S,H,W], union [H,W], owner [H,W]), on the device
    Per step, apart from the network (and the foreground bytes), the launches do not depend on S: track 1, crop 1, bbox 2,
    resolve 1; the frame loop copies nothing to the host -- the log of boxes and origins is read back once, after the last frame.
    Every window size x S is an engine plan of its own and nothing is evicted here (EvalModel.drop_plans between clips).
    Returns dict(alpha [S,T,H,W], alpha_u8, trimap [S,T,3,H,W], union [T,H,W], union_u8, owner [T,H,W] uint8 (255: nobody's),
    bank_frames, roi = per subject [(y0, x0, h, w)] * T, roi_size, roi_clipped = per subject the frames whose box reaches a window
    side that is not the frame's[, fgr_u8]).  Checked by definition only, with synthetic weights (the module's docstring).
    ``key`` (run_video_matte's trimap-free matting of keyed footage) is refused: a key makes ONE mask, not one per subject."""
    if key is not None:
        raise ValueError("%s: key (trimap-free matting of keyed footage) is a single-clip feature (run_video_matte): a key makes one "
                         "mask of the frame, not one per subject" % WHO)
    frames = list(frames) if not (hasattr(frames, "shape") or hasattr(frames, "__getitem__")) else frames
    spec, margin, (H, W) = _refuse(model, frames, subjects, roi, roi_margin, overlap)
    T, S = len(frames), len(subjects)
    if T == 0:
        raise ValueError("%s: the clip has no frames" % WHO)
    core = model.module if hasattr(model, "module") else model
    dev = device or next(core.parameters()).device
    rgb, foreground, normalise = bool(frames_are_rgb), bool(foreground), overlap == "normalise"
    keep = (lambda x: x) if keep_on_device else (lambda x: x.cpu())
    tri_full = [(v.convert(model, dev) if isinstance(v, Mask) else _as_tensor(v).to(dev)).float().contiguous() for v in subjects]
    log = None
    if spec is not None:
        source_rows = bbox(tri_full, torch.empty((S, 8), dtype=torch.int32, device=dev))
        h, w = shared_size([tuple(r[4:]) for r in rows_of(source_rows)], spec, margin, H, W)
        hold = _roi.hold_of(margin)
        log = _roi.new_log((S, T), h, w, dev)                # a row per subject and frame
        tri_dev = None
    else:
        h, w = H, W
        zeros = torch.zeros((S, 2), dtype=torch.int32, device=dev)
        tri_dev = [t[None, None] for t in tri_full]
    want = ("alpha", "alpha_u8", "trimap", "union", "union_u8", "owner") + (("fgr",) if foreground else ())
    names = ("alpha", "alpha_u8", "trimap", "union", "union_u8", "owner")
    kept = {n: [] for n in names}
    rgba, bank, ones = [], [], None
    with _foreground_option(core, foreground):
        for t in range(T):
            f = _as_tensor(frames[t])
            _check_frame(f, t, (H, W))
            ready = getattr(f, "_otvm_ready", None)
            full = f.to(dev, non_blocking=True).contiguous()
            if ready is not None:
                torch.cuda.current_stream(dev).wait_event(ready)
            if log is not None:
                origins = log[:, t, 8:]
                track(source_rows if t == 0 else log[:, t - 1, :8], None if t == 0 else log[:, t - 1, 8:], origins, (h, w), H, W, hold)
                wins, tris = crop(origins, (h, w), frame=full, trimaps=tri_full if t == 0 else None)
                if t == 0:
                    tri_dev = [x[None, None] for x in tris]
            else:
                origins, wins = zeros, [full] * S
            ones = _ones_alpha(ones, h, w, dev)
            memorize, max_memory_num, large = memory_schedule(t, h, w, skip, max_num)
            if foreground:
                core.set_background(None)                     # (the bytes are made behind the resolve, at full resolution)
            outs = core.forward_batch([ones] * S, wins, wins, tri_dev, first_frame=(t == 0), last_frame=(t == T - 1),
                                      memorize=memorize, max_memory_num=max_memory_num, large_input=large, _frames_rgb=rgb)
            tris_out = [o[1][0, 0].contiguous() for o in outs]
            if log is not None:
                bbox(tris_out, log[:, t, :8])                 # what the next frame's windows follow, and roi_clipped's boxes
            res = resolve(origins, (h, w), H, W, [o[3][0, 0, 0] for o in outs], tris_out,
                          core._engine.last_fgr_b if foreground else None, full, rgb, normalise, want)
            if foreground:
                rgba.append(keep(torch.stack([guided.foreground_bytes(res["alpha"][s], res["fgr"][s], rgb, None, WHO)[0]
                                              for s in range(S)])))
            bank.append(list(core.memories["frames"]))
            if on_frame is not None:
                on_frame(t, res["alpha"], res["union"], res["owner"])
            for n in names:
                kept[n].append(keep(res[n]))
    out = {n: torch.stack(kept[n], dim=1 if n in ("alpha", "alpha_u8", "trimap") else 0) for n in names}
    out["bank_frames"] = bank
    if foreground:
        out["fgr_u8"] = torch.stack(rgba, dim=1)
    out.update(_windows(log, S, T, H, W, h, w))
    return out


def _windows(log, S, T, H, W, h, w):
    """roi, roi_size and roi_clipped per subject (ONE read-back of the log, after the last frame; none without windows)"""
    if log is None:
        return dict(roi=[[(0, 0, H, W)] * T for _ in range(S)], roi_size=(H, W), roi_clipped=[[] for _ in range(S)])
    per_subject = [_roi.clipped(rows, (h, w), H, W, range(T)) for rows in rows_of(log)]
    return dict(roi=[wins for wins, _ in per_subject], roi_size=(h, w), roi_clipped=[cut for _, cut in per_subject])
