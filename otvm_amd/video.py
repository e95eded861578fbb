"""``run_video_matte``: the build-owned counterpart of the reference's per-sequence loop
(reference eval.py:157-228) -- frame flags, memory schedule, large-input rule, u8 quantisation.

BASELINE.json names a ``run_video_matte()`` call surface; the reference has no such function (its loop
is inlined in eval.py), so this reproduces that loop around the reference-shaped ``EvalModel``.
"""
import contextlib

import numpy as np
import torch

from .masks import Mask, as_mask


def memory_schedule(i_seq, height, width, skip=10, max_num=5):
    """(memorize, max_memory_num, large_input) for frame ``i_seq`` -- eval.py:180-190, config.py:22-23."""
    large = min(height, width) > 1100
    if large:
        skip, max_num = int(skip * 2), int(max_num / 2)
    memorize = (i_seq % skip) == 0 if skip > 2 else False
    return memorize, max_num, large


def _keyframe_kind(v):
    """"key" (a full trimap: one-hot [3,H,W]) or "labels" (a uint8 [H,W] label map) of one entry of ``keyframes``."""
    if isinstance(v, Mask):                           # a mask in a trimap's ("key") or a label map's ("labels") place
        return v.role
    if isinstance(v, str):
        if v not in ("key", "labels"):
            raise ValueError("keyframes: an entry is a one-hot trimap [3,H,W], a uint8 label map [H,W], 'key' or 'labels'; got %r" % v)
        return v
    nd = v.dim() if torch.is_tensor(v) else np.asarray(v).ndim
    if nd not in (2, 3):
        raise ValueError("keyframes: an entry is a one-hot trimap [3,H,W] or a uint8 label map [H,W], got %d dimensions" % nd)
    return "key" if nd == 3 else "labels"


def keyframe_schedule(T, keyframes, skip=10):
    """Order in which a clip of ``T`` frames with trimaps / label maps on several frames is matted (pure host function).

    keyframes: {frame: one-hot trimap [3,H,W] (a FULL keyframe) | uint8 label map [H,W] (a correction)}; the strings "key" /
    "labels" stand for the arrays.  Returns the steps (t, kind, first_frame, last_frame, memorize), kind in "key" / "labels" /
    "frame".  With k0 the earliest full keyframe (there must be one):
      A. every full keyframe in ascending order, k0 as the clip's first_frame, the others as keyframe steps: all of them are in
         the memory bank -- as anchors -- before any other frame is matted;
      B. forward over k0+1 .. T-1 without the full keyframes (their outputs exist), memorize = (t - k0) % skip == 0;
      C. backward over k0-1 .. 0 (the driver first drops every slot that is not an anchor), memorize = (k0 - t) % skip == 0.
    Only the last step issued carries last_frame.  A label map is applied at its frame in either sweep.  ``skip`` is the
    effective one (memory_schedule's large-input rule applied by the caller); skip <= 2 never memorises (eval.py:186-189).
    keyframes = {0: trimap} gives eval.py:178-189 exactly."""
    kinds = {int(t): _keyframe_kind(v) for t, v in keyframes.items()}
    for t in kinds:
        if not 0 <= t < T:
            raise ValueError("keyframes: frame %d lies outside the clip (%d frames)" % (t, T))
    keys = sorted(t for t, k in kinds.items() if k == "key")
    if not keys:
        raise ValueError("keyframes: at least one full keyframe (a one-hot trimap [3,H,W]) is required")
    k0 = keys[0]

    def mem(d):
        return (d % skip) == 0 if skip > 2 else False
    steps = [(k, "key", k == k0, False, mem(k - k0)) for k in keys]
    steps += [(t, kinds.get(t, "frame"), False, False, mem(t - k0)) for t in range(k0 + 1, T) if kinds.get(t) != "key"]
    steps += [(t, kinds.get(t, "frame"), False, False, mem(k0 - t)) for t in range(k0 - 1, -1, -1)]
    t, kind, first, _, m = steps[-1]
    steps[-1] = (t, kind, first, True, m)
    return steps


def trimap_file_to_onehot(tri):
    """Grayscale / 3-channel trimap image -> one-hot float32 [3,H,W] (bg, unknown, fg): dataset.py:880-893."""
    tri = np.asarray(tri)
    if tri.ndim == 3:
        t = tri[..., :3] > 1                           # BGR order as read by cv2 (an alpha plane carries no class)
        out = np.zeros(t.shape, np.float32)
        out[..., 0][np.logical_not(t[..., 1] + t[..., 2])] = 1
        out[..., 1][t[..., 2]] = 1
        out[..., 2][t[..., 1]] = 1
    else:
        t = tri.copy()
        out = np.zeros(t.shape + (3,), np.float32)
        out[..., 0][t == 0] = 1
        out[..., 2][t == t.max()] = 1
        t[t == t.max()] = 0
        out[..., 1][t == t.max()] = 1                  # second-largest level = unknown (incl. the two-level quirk)
    return np.ascontiguousarray(out.transpose(2, 0, 1))


@torch.no_grad()
def _as_tensor(x):
    """numpy / tensor -> tensor without the read-only-array warning (PIL hands out non-writable buffers)."""
    if torch.is_tensor(x):
        return x
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def _background_at(spec, i, dev, cache):
    """Entry ``i`` of a ``new_background``: a TUPLE is a colour triple and an array / tensor [H,W,3] one image, either serving
    every frame; a LIST (or a [T,H,W,3] array) holds one of those per frame.  An image that serves every frame is uploaded once."""
    per_frame = isinstance(spec, list) or (hasattr(spec, "ndim") and spec.ndim == 4)
    x = spec[i] if per_frame else spec
    if isinstance(x, tuple):
        return x
    if not per_frame and "image" in cache:
        return cache["image"]
    t = _as_tensor(x)
    if t.dtype != torch.uint8:
        raise ValueError("run_video_matte: a new background image is uint8 [H,W,3], got %s" % t.dtype)
    t = t.to(dev).contiguous()
    if not per_frame:
        cache["image"] = t
    return t


@contextlib.contextmanager
def _foreground_option(core, on):
    """EvalModel.foreground = True for the clip (when asked for); the model's option and background are restored afterwards."""
    if not on:
        yield
        return
    saved = (core.foreground, core._background)
    core.foreground = True
    try:
        yield
    finally:
        core.foreground, core._background = saved


def run_video_matte(model, frames, trimap=None, alphas=None, backgrounds=None, skip=10, max_num=5,
                    frames_are_rgb=False, on_frame=None, device=None, keep_on_device=False, gt_alpha_u8=None,
                    gt_mask_u8=None, gt_mask=None, gt_image_metrics=False, gt_flow_metrics=False, foreground=False,
                    new_background=None, keyframes=None, work_scale=None, work_radius=2, work_eps=1e-4, on_foreground=None,
                    mask=None, masks=None):
    """Matte one sequence.

    model       : EvalModel (optionally wrapped in nn.DataParallel), on the GPU
    frames      : iterable/array of uint8 or float [H,W,3] images, BGR (cv2 order) unless frames_are_rgb
    trimap      : first-frame trimap, one-hot float [3,H,W] (demo flow, dataset.py:866-893) or None
    alphas      : per-frame GT alpha [H,W] in [0,1] (VideoMatting108 flow: first-frame trimap derived
                  from alpha with the model's dilate kernel) -- required when trimap is None
    gt_alpha_u8 : optional per-frame ground-truth alpha, uint8 [H,W]; with it SAD/MSE/dtSSD are accumulated on
                  the device (ClipMetrics) and returned under "metrics"; gt_mask_u8 = optional {0,1} evaluation masks,
                  gt_mask="unknown" = the reference metric's default mask (0 < gt < 255) instead; gt_image_metrics=True adds
                  Grad, Conn and SSDA (ClipMetrics(image_metrics=True)), gt_flow_metrics=True MESSDdt
                  (ClipMetrics(flow_metrics=True))
    backgrounds : optional per-frame BG images (V108 composites fg*a + bg*(1-a)), same dtype / channel order as the
                  frames; default bg = fg
    foreground  : also return the network's foreground estimate as straight-alpha RGBA: "fgr_u8" [T,H,W,4] uint8, colour in
                  the frames' channel order, A = alpha_u8 (EvalModel.foreground; the model's option is restored afterwards)
    new_background : composite that foreground over a new background -> "comp_u8" [T,H,W,3].  A tuple (c0, c1, c2) is a
                  colour, a uint8 [H,W,3] array / tensor an image of the frames' resolution, a list one of those per frame;
                  all in the frames' channel order (switches ``foreground`` on: the composite needs F)
    keyframes   : {frame: one-hot trimap [3,H,W] | uint8 label map [H,W] (0 bg, 1 unknown, 2 fg, 255 unlabelled)}, together
                  with or instead of ``trimap`` (= {0: trimap}).  A trimap makes its frame a FULL keyframe (matted from that
                  trimap, memorised as an anchor slot the bank never evicts), a label map a correction of the propagated trimap.
                  The clip is matted in the order of keyframe_schedule -- the keyframes, then forward from the earliest one,
                  then backward from it to frame 0 -- so ``frames`` must allow random access; on_frame fires in that order
                  with the frame's index.  Everything returned (and the metrics) is in natural frame order.
    on_foreground : callable(i, rgba_u8 [H,W,4], comp_u8 [H,W,3] or None), fired per frame after on_frame when ``foreground`` is
                  on.  The frames are then handed over instead of being collected: the result has no "fgr_u8" / "comp_u8" (a
                  writer consumes them as they come; nothing of a long clip piles up on the device)
    work_scale  : 2, 3 or 4: working-resolution matting.  The frames (uint8 [H,W,3] only) are reduced on the device to
                  h x w = ceil(H / s) x ceil(W / s) by block means, the network runs there -- ``trimap`` and the entries of
                  ``keyframes`` are given at H x W and reduced conservatively (otvm_amd/guided.py) -- and alpha (with ``foreground``
                  also F) returns to H x W through a guided filter on the full-resolution frame of radius ``work_radius`` (1 ... 4,
                  in working pixels) and regulariser ``work_eps`` ([0,1] scale).  The defaults of the two are PLACEHOLDERS: nobody
                  has tuned them on real footage.  alpha, alpha_u8, fgr_u8, comp_u8, on_frame's alpha / u8 and the metrics are at
                  H x W (``new_background`` too); ``trimap`` comes back at the working resolution [T,3,h,w], the result gains
                  work_size=(h, w), and the memory schedule (large-input rule included) is evaluated at h x w, which is what the
                  model runs.  Not available for float frames, the ``alphas`` flow, ``backgrounds`` or run_video_matte_batch.
    mask        : a segmentation mask of the first frame in ``trimap``'s place: an array / tensor [H,W] (uint8, or float in
                  [0,1]; binary or soft) or a masks.Mask carrying its band and thresholds.  The trimap is made on the device
                  (otvm_trimap_from_mask: the thresholded mask eroded by exact Euclidean discs; the band defaults to the model's
                  DILATION_KERNEL, the thresholds to a binary cut -- PLACEHOLDERS nobody tuned on real footage).  The entries of
                  ``keyframes`` may be Masks too: role="key" a full keyframe, role="labels" a correction whose band stays
                  unlabelled.  Every mask is converted once per clip, at H x W (before the reduction of ``work_scale``); the band
                  is in full-resolution pixels.
    masks       : one mask per frame (a sequence of T arrays or Masks, role "key"): every frame is matted from its own mask and
                  NOTHING is propagated -- each step runs as a clip of one frame (first_frame and last_frame), in natural order,
                  so the STM query encoder, memory read, decoder and Encoder_M never run and the bank stays empty (bank_frames
                  is [] for every frame).  Exclusive with trimap, mask, keyframes and alphas; on_frame, the metrics, foreground
                  and new_background work as in any clip.  Not available in run_video_matte_batch.
    Returns dict(alpha=[T,H,W] float32, alpha_u8=[T,H,W] uint8 (truncated, eval.py:209), trimap=[T,3,H,W],
    bank_frames=[per frame: ids of the frames resident in the memory bank after that frame's update]) and, when ``keyframes``
    was given, anchor_frames=[per frame: those of them that are anchors], schedule=[the steps issued, keyframe_schedule's tuples].
    """
    if work_scale is not None:
        from . import guided
        if work_scale not in guided.SCALES:
            raise ValueError("run_video_matte: work_scale is 2, 3 or 4 (an integer scale), got %r" % (work_scale,))
        if work_radius not in guided.RADII:
            raise ValueError("run_video_matte: work_radius is 1 ... 4, got %r" % (work_radius,))
        if not work_eps > 0:
            raise ValueError("run_video_matte: work_eps must be positive, got %r" % (work_eps,))
        if alphas is not None:
            raise ValueError("run_video_matte: work_scale belongs to the trimap flow; the alphas flow (VideoMatting108: trimaps "
                             "from ground-truth alpha) has no working-resolution route")
        if backgrounds is not None:
            raise ValueError("run_video_matte: work_scale takes no per-frame `backgrounds` (they belong to the alphas flow)")
    frames = list(frames) if not (hasattr(frames, "shape") or hasattr(frames, "__getitem__")) else frames
    T = len(frames)
    dev = device or next(model.parameters()).device
    mask_hw = {}                                      # frame -> the size of the mask it was given (checked against the frame)
    if mask is not None or masks is not None:
        if masks is not None:
            for name, other in (("trimap", trimap), ("mask", mask), ("keyframes", keyframes), ("alphas", alphas)):
                if other is not None:
                    raise ValueError("run_video_matte: `masks` mattes every frame from its own mask and excludes `%s`" % name)
            masks = [as_mask(m, "run_video_matte: masks[%d]" % j) for j, m in enumerate(masks)]
            if len(masks) != T:
                raise ValueError("run_video_matte: `masks` needs one mask per frame, got %d for %d frames" % (len(masks), T))
            if any(m.role != "key" for m in masks):
                raise ValueError("run_video_matte: a Mask of `masks` has role 'key' (role='labels' corrects a PROPAGATED trimap; "
                                 "nothing is propagated here)")
            for m in masks:
                m.band_for(model)                         # (a missing band is refused before any frame runs)
        if mask is not None:
            if trimap is not None:
                raise ValueError("run_video_matte: frame 0 has both `trimap` and `mask`")
            if alphas is not None:
                raise ValueError("run_video_matte: `mask` belongs to the trimap flow (no per-frame alphas)")
            if keyframes is not None and 0 in {int(t) for t in keyframes}:
                raise ValueError("run_video_matte: frame 0 has both `mask` and an entry of `keyframes`")
            trimap = as_mask(mask, "run_video_matte: mask")
            if trimap.role != "key":
                raise ValueError("run_video_matte: `mask` is the first frame's trimap: a Mask with role 'key' (role='labels' "
                                 "corrects a propagated trimap on a later frame)")
    ups, work_hw = None, None
    # (a plain sequence is checked before anything is uploaded; a streaming source is checked frame by frame below)
    if (work_scale is not None and T > 0 and (isinstance(frames, (list, tuple, np.ndarray)) or torch.is_tensor(frames))
            and _as_tensor(frames[0]).dtype != torch.uint8):
        raise ValueError("run_video_matte: work_scale takes uint8 [H,W,3] frames (float frames have no working-resolution "
                         "route), got %s" % _as_tensor(frames[0]).dtype)
    out_a, out_u8, out_t, bank_log, anchor_log = [None] * T, [None] * T, [None] * T, [None] * T, [None] * T
    out_f, out_c, bg_cache = [None] * T, [None] * T, {}
    core = model.module if hasattr(model, "module") else model
    foreground = bool(foreground) or new_background is not None
    metrics = (ClipMetrics(dev, image_metrics=gt_image_metrics, flow_metrics=gt_flow_metrics) if gt_alpha_u8 is not None
               else None)
    # loop invariants: the user trimap (25 MB as fp32 at 1080p) is uploaded once, not once per frame; the dummy alpha
    # of the trimap flow is one tensor for the whole clip
    keyed = keyframes is not None                     # the caller asked for keyframes: the result carries the extra keys
    if keyframes is not None:
        if alphas is not None:
            raise ValueError("run_video_matte: keyframes belong to the trimap flow (no per-frame alphas)")
        keyframes = {int(t): v for t, v in keyframes.items()}
        if trimap is not None:
            if 0 in keyframes:
                raise ValueError("run_video_matte: frame 0 has both `trimap` and an entry of `keyframes`")
            keyframes[0] = trimap
    elif trimap is not None:
        keyframes = {0: trimap}
    if keyframes is not None and T > 0:
        # masks become ordinary trimaps / label maps here, once per clip, at the resolution they were given
        for t, v in list(keyframes.items()):
            if isinstance(v, Mask):
                mask_hw[t] = v.shape
                keyframes[t] = v.convert(model, dev)
    tri_devs, lab_devs, steps, k0 = {}, {}, None, 0
    if keyframes is not None and T > 0:
        for t, v in keyframes.items():
            if _keyframe_kind(v) == "key":
                tri_devs[t] = _as_tensor(v).to(dev).float()
                if work_scale is not None:
                    tri_devs[t] = guided.downsample_trimap(tri_devs[t], work_scale)
                tri_devs[t] = tri_devs[t][None, None]
            else:
                lab_devs[t] = _as_tensor(v).to(dev)
                if work_scale is not None:
                    lab_devs[t] = guided.downsample_labels(lab_devs[t], work_scale)
        if not tri_devs:
            raise ValueError("run_video_matte: keyframes need at least one full trimap (one-hot [3,H,W])")
        k0 = min(tri_devs)
        # the schedule takes the effective skip: the large-input rule needs the resolution, which the trimaps carry
        large = memory_schedule(0, tri_devs[k0].shape[-2], tri_devs[k0].shape[-1], skip, max_num)[2]
        steps = keyframe_schedule(T, {t: "key" for t in tri_devs} | {t: "labels" for t in lab_devs},
                                  int(skip * 2) if large else skip)
    elif masks is not None and T > 0:
        steps = [(i, "key", True, True, False) for i in range(T)]                   # T clips of one frame: nothing to memorise
        mask_hw = {i: m.shape for i, m in enumerate(masks)}
    elif T > 0:
        steps = [(i, "frame", i == 0, i == T - 1, None) for i in range(T)]          # alpha flow: eval.py's loop as it is
    natural = steps is None or all(st[0] == j for j, st in enumerate(steps))
    ones = None
    with _foreground_option(core, foreground):
        for i, kind, first_frame, last_frame, step_memorize in (steps or []):
            f = _as_tensor(frames[i])
            b = _as_tensor(backgrounds[i]) if backgrounds is not None else None
            extra = {}
            if work_scale is not None:
                if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
                    raise ValueError("run_video_matte: work_scale takes uint8 [H,W,3] frames (float frames have no "
                                     "working-resolution route), got %s %s" % (f.dtype, tuple(f.shape)))
                ready = getattr(f, "_otvm_ready", None)
                full = f.to(dev, non_blocking=True).contiguous()
                if ready is not None:
                    torch.cuda.current_stream(dev).wait_event(ready)     # the reduction below reads the upload on this stream
                if ups is None or (ups.H, ups.W) != tuple(full.shape[:2]):
                    ups = guided.GuidedUpsampler(dev, full.shape[0], full.shape[1], work_scale, work_radius, work_eps,
                                                 4 if foreground else 1)
                    work_hw = (ups.h, ups.w)
                fg = bg = ups.reduce(full)
                H, W = work_hw
                full_hw = tuple(full.shape[:2])
                extra["_frames_rgb"] = bool(frames_are_rgb)
            elif f.dtype == torch.uint8 and (b is None or b.dtype == torch.uint8):
                # decoded images go to the device as they are ([H,W,3] uint8): the preprocess kernel converts, flips the
                # channel order and composites -- no per-frame torch conversion / transposition kernels
                ready = getattr(f, "_otvm_ready", None)           # upload event of the IO pipeline's prefetcher
                fg = f.to(dev, non_blocking=True)
                bg = fg if b is None else b.to(dev, non_blocking=True)
                if b is not None and getattr(b, "_otvm_ready", None) is not None:
                    torch.cuda.current_stream(dev).wait_event(b._otvm_ready)
                H, W = fg.shape[:2]
                full_hw = (H, W)
                extra["_frames_rgb"] = bool(frames_are_rgb)
                if ready is not None:
                    # the upload event may only travel to the model (whose query-encoder stream then starts on it, ahead of the
                    # launch stream) when EVERYTHING the preprocess reads is covered by it or loop-invariant: the frame itself
                    # (no copy made here), no separately uploaded background, and the trimap flow's constant alpha -- a per-frame
                    # alpha is written by the launch stream just below.  Otherwise the launch stream waits for the upload
                    # and the model orders its side streams behind the launch stream.
                    if b is None and fg is f and keyframes is not None:
                        extra["_inputs_ready"] = ready
                    else:
                        torch.cuda.current_stream(dev).wait_event(ready)
            else:
                f = f.to(dev).float()
                if frames_are_rgb:
                    f = f.flip(-1)
                fg = f.permute(2, 0, 1)[None, None].contiguous()
                H, W = fg.shape[-2:]
                if b is not None:                                 # backgrounds come in the same channel order as the frames
                    b = b.to(dev).float()
                    if frames_are_rgb:
                        b = b.flip(-1)
                    bg = b.permute(2, 0, 1)[None, None].contiguous()
                else:
                    bg = fg
                full_hw = (H, W)
            # masks of a keyframe clip are all held against the first frame that comes by, those of `masks` each against its own
            for t in ([i] if masks is not None else list(mask_hw)):
                hw = mask_hw.pop(t)
                if tuple(hw) != tuple(full_hw):
                    raise ValueError("run_video_matte: the mask of frame %d is %dx%d, the frames are %dx%d (masks are given at "
                                     "the frames' resolution)" % (t, hw[0], hw[1], full_hw[0], full_hw[1]))
            if masks is not None:
                if ones is None or ones.shape[-2:] != (H, W):
                    ones = torch.ones(1, 1, 1, H, W, device=dev)
                tri_gt = masks[i].convert(model, dev)             # this frame's own trimap; nothing is kept of it
                if work_scale is not None:
                    tri_gt = guided.downsample_trimap(tri_gt, work_scale)
                a, tri_gt = ones, tri_gt[None, None]
            elif keyframes is not None:
                if ones is None or ones.shape[-2:] != (H, W):
                    ones = torch.ones(1, 1, 1, H, W, device=dev)
                # (as eval.py does, every frame is handed a trimap -- it comes back as out[2]; only a keyframe consumes it)
                a, tri_gt = ones, tri_devs.get(i, tri_devs[k0])
                if kind == "key" and not first_frame:
                    extra["keyframe"] = True
                elif kind == "labels":
                    extra["labels"] = lab_devs[i]
                if i == k0 - 1:
                    core.drop_non_anchors()                       # the backward sweep starts from the keyframes alone
            else:
                al = alphas[i]
                al = _as_tensor(al)
                a = al.to(dev).float()[None, None, None]
                tri_gt = None
            memorize, max_memory_num, large = memory_schedule(i, H, W, skip, max_num)
            if step_memorize is not None:
                memorize = step_memorize
            if foreground:
                # (working resolution: the composite is made at full resolution below, not by the engine)
                core.set_background(None if new_background is None or ups is not None
                                    else _background_at(new_background, i, dev, bg_cache))
            out = model(a, fg, bg, tri=None, tri_gt=tri_gt, first_frame=first_frame, last_frame=last_frame,
                        memorize=memorize, max_memory_num=max_memory_num, large_input=large, _frame_id=i, **extra)
            alpha = out[3][0, 0, 0]
            u8 = core._engine.last_alpha_u8
            rgba = comp = None
            if ups is not None:
                # guided upsampling on this stream, behind the frame: the guide is the working frame the network saw
                alpha, u8, fgr_full = ups.upsample(full, fg, [alpha] + (list(core._engine.last_fgr) if foreground else []))
                if foreground:
                    nb = None if new_background is None else _background_at(new_background, i, dev, bg_cache)
                    if isinstance(nb, tuple) and not (len(nb) == 3 and all(0 <= int(x) <= 255 for x in nb)):
                        raise ValueError("run_video_matte: a background colour is three values in 0..255, got %r" % (nb,))
                    rgba, comp = ups.foreground_bytes(alpha, fgr_full, frames_are_rgb, nb)
            elif foreground:
                rgba, comp = core._engine.last_rgba_u8, core._engine.last_comp_u8
            mem_now = core.memories                                 # frame ids resident after this frame's update (host lists)
            bank_log[i], anchor_log[i] = list(mem_now["frames"]), list(mem_now["anchors"])
            if metrics is not None and natural:
                _metrics_add(metrics, u8, i, gt_alpha_u8, gt_mask_u8, gt_mask, dev)
            if on_frame is not None:
                on_frame(i, alpha, u8, out)
            if keep_on_device:
                out_a[i], out_u8[i], out_t[i] = alpha, u8, out[1][0, 0]
            else:
                out_a[i], out_u8[i], out_t[i] = alpha.cpu(), u8.cpu(), out[1][0, 0].cpu()
            if foreground and on_foreground is not None:
                on_foreground(i, rgba, comp)
            elif foreground:
                out_f[i] = rgba if keep_on_device else rgba.cpu()
                if new_background is not None:
                    out_c[i] = comp if keep_on_device else comp.cpu()
    if metrics is not None and not natural:
        # the pair terms (dtSSD, MESSDdt) depend on the order: fed in natural frame order from the kept 8-bit alphas
        for i in range(T):
            _metrics_add(metrics, out_u8[i].to(dev), i, gt_alpha_u8, gt_mask_u8, gt_mask, dev)
    res = dict(alpha=torch.stack(out_a), alpha_u8=torch.stack(out_u8), trimap=torch.stack(out_t), bank_frames=bank_log)
    if keyed:
        res.update(anchor_frames=anchor_log, schedule=list(steps or []))
    if work_scale is not None:
        res["work_size"] = work_hw
    if foreground and on_foreground is None:
        res["fgr_u8"] = torch.stack(out_f)
        if new_background is not None:
            res["comp_u8"] = torch.stack(out_c)
    if metrics is not None:
        res["metrics"] = metrics.result()
    return res


def _metrics_add(metrics, u8, i, gt_alpha_u8, gt_mask_u8, gt_mask, dev):
    g = _as_tensor(gt_alpha_u8[i])
    mk = gt_mask
    if gt_mask_u8 is not None:
        mk = _as_tensor(gt_mask_u8[i]).to(dev)
    metrics.add(u8, g.to(dev), mk)


def run_video_matte_batch(model, clips, trimaps=None, alphas=None, backgrounds=None, skip=10, max_num=5, frames_are_rgb=False,
                          device=None, keep_on_device=False, on_frame=None, gt_alpha_u8=None, gt_mask=None,
                          gt_image_metrics=False, gt_flow_metrics=False, foreground=False, new_background=None, keyframes=None,
                          work_scale=None, mask=None, masks=None):
    """Matte B sequences of one resolution in LOCK-STEP (round 3): frame i of every clip goes through the network in one
    batched step (EvalModel.forward_batch: one launch per layer over the B images, per-sequence memory banks).
    clips: list of B frame arrays ([T_b,H,W,3] uint8 / float, BGR unless frames_are_rgb); trimaps: list of B first-frame
    one-hot trimaps [3,H,W] (demo flow) or None with alphas = list of B per-frame GT alpha lists (V108 flow: the first-frame
    trimap is derived from the alpha); backgrounds: optional list of B per-frame background lists; gt_alpha_u8: optional
    list of B per-frame uint8 ground truths (SAD / MSE / dtSSD per clip, as run_video_matte; gt_image_metrics=True adds Grad,
    Conn and SSDA, gt_flow_metrics=True MESSDdt); on_frame(b, i, alpha, u8, out).
    Clips may differ in LENGTH: the batch runs max(T_b) steps, a clip that has ended keeps feeding its last frame (its
    outputs from then on are discarded) -- sequences are independent (all recurrent state is per sequence), so
    this changes no result of the others; the frame flags follow the frame index, which the clips share.
    Each returned dict's alpha / alpha_u8 / trimap / metrics equal run_video_matte of that clip alone (bit for bit under the
    same kernel configurations).  bank_frames follows the SHARED schedule: ``last_frame`` is keyed to the longest clip, so a
    shorter clip's final entry still lists the frame whose memorize is pending -- the stand-alone run, whose last frame
    memorises nothing, does not (the one documented difference).
    foreground / new_background: as run_video_matte ("fgr_u8" [T_b,H,W,4], "comp_u8" [T_b,H,W,3] per clip); new_background = a
    list of B entries, one per clip, each what run_video_matte takes (colour tuple, image, or per-frame list).
    Returns a list of B dicts (alpha, alpha_u8, trimap, bank_frames[, metrics][, fgr_u8][, comp_u8])."""
    if keyframes is not None:
        raise NotImplementedError("run_video_matte_batch: keyframes are a single-clip feature (run_video_matte)")
    if work_scale is not None:
        raise ValueError("run_video_matte_batch: work_scale (working-resolution matting) is a single-clip feature "
                         "(run_video_matte); lock-step batches run at the frames' resolution")
    if mask is not None or masks is not None or (trimaps is not None and any(isinstance(t, Mask) for t in trimaps)):
        raise ValueError("run_video_matte_batch: trimaps from masks (mask / masks / a Mask) are a single-clip feature "
                         "(run_video_matte); lock-step batches take trimaps")
    B = len(clips)
    lens = [len(c) for c in clips]
    T = max(lens)
    if (trimaps is None) == (alphas is None):
        raise ValueError("run_video_matte_batch: give either trimaps (demo flow) or alphas (VideoMatting108 flow)")
    core = model.module if hasattr(model, "module") else model
    dev = device or next(core.parameters()).device
    res = [dict(alpha=[], alpha_u8=[], trimap=[], bank_frames=[], fgr_u8=[], comp_u8=[]) for _ in range(B)]
    foreground = bool(foreground) or new_background is not None
    if new_background is not None and not (isinstance(new_background, list) and len(new_background) == B):
        raise ValueError("run_video_matte_batch: new_background is a list of one entry per clip")
    bg_cache = [{} for _ in range(B)]
    metrics = ([ClipMetrics(dev, image_metrics=gt_image_metrics, flow_metrics=gt_flow_metrics) for _ in range(B)]
               if gt_alpha_u8 is not None else None)
    tri_dev = None if trimaps is None else [_as_tensor(t).to(dev).float()[None, None] for t in trimaps]
    ones = None
    with _foreground_option(core, foreground):
        for i in range(T):
            A, FG, BG = [], [], []
            for b in range(B):
                j = min(i, lens[b] - 1)                               # a clip that has ended repeats its last frame (discarded)
                f = _as_tensor(clips[b][j])
                bk = _as_tensor(backgrounds[b][j]) if backgrounds is not None else None
                if f.dtype == torch.uint8 and (bk is None or bk.dtype == torch.uint8):
                    fg = f.to(dev, non_blocking=True)
                    bg = fg if bk is None else bk.to(dev, non_blocking=True)
                    # frames handed over by the IO pipeline's prefetcher carry their upload event: the launch stream waits for
                    # it before anything reads them (as run_video_matte does; the batched step makes no promise to the engine
                    # about its inputs, so its side streams order themselves behind the launch stream)
                    for src in (f, bk):
                        ev = getattr(src, "_otvm_ready", None) if src is not None else None
                        if ev is not None:
                            torch.cuda.current_stream(dev).wait_event(ev)
                    H, W = fg.shape[:2]
                    rgb = bool(frames_are_rgb)
                else:
                    f = f.to(dev).float()
                    if frames_are_rgb:
                        f = f.flip(-1)
                    fg = f.permute(2, 0, 1)[None, None].contiguous()
                    H, W = fg.shape[-2:]
                    if bk is not None:
                        bk = bk.to(dev).float()
                        if frames_are_rgb:
                            bk = bk.flip(-1)
                        bg = bk.permute(2, 0, 1)[None, None].contiguous()
                    else:
                        bg = fg
                    rgb = False
                if trimaps is not None:
                    if ones is None or ones.shape[-2:] != (H, W):
                        ones = torch.ones(1, 1, 1, H, W, device=dev)
                    a = ones
                else:
                    a = _as_tensor(alphas[b][j]).to(dev).float()[None, None, None]
                A.append(a), FG.append(fg), BG.append(bg)
            memorize, max_memory_num, large = memory_schedule(i, H, W, skip, max_num)
            if foreground:
                core.set_background(None if new_background is None else
                                    [_background_at(new_background[b], min(i, lens[b] - 1), dev, bg_cache[b]) for b in range(B)])
            outs = core.forward_batch(A, FG, BG, tri_dev if tri_dev is not None else [None] * B, first_frame=(i == 0),
                                      last_frame=(i == T - 1), memorize=memorize, max_memory_num=max_memory_num, large_input=large,
                                      _frames_rgb=rgb)
            u8s = core._engine.last_alpha_u8_b
            bank = list(core.memories["frames"])
            for b in range(B):
                if i >= lens[b]:
                    continue
                al, u8, tr = outs[b][3][0, 0, 0], u8s[b], outs[b][1][0, 0]
                if metrics is not None:
                    metrics[b].add(u8, _as_tensor(gt_alpha_u8[b][i]).to(dev), gt_mask)
                if on_frame is not None:
                    on_frame(b, i, al, u8, outs[b])
                if not keep_on_device:
                    al, u8, tr = al.cpu(), u8.cpu(), tr.cpu()
                res[b]["alpha"].append(al), res[b]["alpha_u8"].append(u8), res[b]["trimap"].append(tr)
                res[b]["bank_frames"].append(bank)
                if foreground:
                    eng = core._engine
                    res[b]["fgr_u8"].append(eng.last_rgba_u8_b[b] if keep_on_device else eng.last_rgba_u8_b[b].cpu())
                    if new_background is not None:
                        res[b]["comp_u8"].append(eng.last_comp_u8_b[b] if keep_on_device else eng.last_comp_u8_b[b].cpu())
    out = []
    for b, r in enumerate(res):
        d = dict(alpha=torch.stack(r["alpha"]), alpha_u8=torch.stack(r["alpha_u8"]), trimap=torch.stack(r["trimap"]),
                 bank_frames=r["bank_frames"])
        if metrics is not None:
            d["metrics"] = metrics[b].result()
        if foreground:
            d["fgr_u8"] = torch.stack(r["fgr_u8"])
            if new_background is not None:
                d["comp_u8"] = torch.stack(r["comp_u8"])
        out.append(d)
    return out


class ClipMetrics:
    """SAD / MSE / dtSSD of a clip accumulated on the device (otvm_matting_metrics), reference definitions
    utils/tmp/metric.py:177-189,252-264 on the 8-bit alphas the path writes (eval.py:209).  One row of partial sums
    per frame stays on the device (no per-frame synchronisation); result() turns them into the reference's per-frame
    values.  mask: None = all pixels, "unknown" = the reference's default (0 < target < 255, metric.py:113-115), or
    explicit uint8 {0,1} masks.
    image_metrics=True also runs otvm_matting_grad_conn per frame into a second row buffer on the same stream: result()
    then adds Grad and Conn (BatchGradient / BatchConnectivity, metric.py:191-234, as they return them: no /1000) and SSDA
    (metric.py:244-250: sqrt of the masked squared error / 255 and its count, from the SAD / MSE row).
    flow_metrics=True also runs otvm_matting_messddt on each pair (previous, current frame) into a third row buffer on the
    same stream: result() then adds MESSDdt (metric.py:266-302: Farneback flow of the ground truth, the reference's
    transposed lookup) per pair with its count, as dtSSD."""

    def __init__(self, device, capacity=256, image_metrics=False, flow_metrics=False):
        from . import lib as L
        self.L, self.lib = L, L.load()
        self.device = device
        self.acc = torch.zeros(capacity, 5, dtype=torch.float64, device=device)
        self.image_metrics = bool(image_metrics)
        self.acc_gc = torch.zeros(capacity, 2, dtype=torch.float64, device=device) if self.image_metrics else None
        self.flow_metrics = bool(flow_metrics)
        self.acc_fl = torch.zeros(capacity, 2, dtype=torch.float64, device=device) if self.flow_metrics else None
        self.ws, self.ws_shape = None, None
        self.ws_fl, self.ws_fl_shape = None, None
        self.prev = None
        self.frames = 0

    def add(self, pred_u8, target_u8, mask_u8=None):
        """pred/target: uint8 [H,W] device tensors (0..255); mask: uint8 {0,1}, "unknown" or None (all pixels)."""
        st = torch.cuda.current_stream(pred_u8.device).cuda_stream
        pred_u8, target_u8 = pred_u8.contiguous(), target_u8.contiguous()
        if isinstance(mask_u8, str):
            if mask_u8 != "unknown":
                raise ValueError("ClipMetrics: mask must be None, 'unknown' or a uint8 tensor")
            mask_u8 = ((target_u8 > 0) & (target_u8 < 255)).to(torch.uint8)
        mask_u8 = None if mask_u8 is None else mask_u8.contiguous()
        if self.frames == self.acc.shape[0]:
            self.acc = torch.cat([self.acc, torch.zeros_like(self.acc)])
            if self.acc_gc is not None:
                self.acc_gc = torch.cat([self.acc_gc, torch.zeros_like(self.acc_gc)])
            if self.acc_fl is not None:
                self.acc_fl = torch.cat([self.acc_fl, torch.zeros_like(self.acc_fl)])
        pp, tp, mp = self.prev if self.prev is not None else (None, None, None)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        self.L.check(self.lib.otvm_matting_metrics(ptr(pred_u8), ptr(target_u8), ptr(mask_u8), ptr(pp), ptr(tp), ptr(mp),
                                                   pred_u8.numel(), self.acc[self.frames].data_ptr(), st), "matting_metrics")
        if self.image_metrics:
            H, W = pred_u8.shape[-2:]
            if self.ws_shape != (H, W):            # stream-ordered re-use: the previous frame's launches come first
                self.ws = torch.empty(self.lib.otvm_matting_grad_conn_ws_bytes(H, W), dtype=torch.uint8, device=pred_u8.device)
                self.ws_shape = (H, W)
            self.L.check(self.lib.otvm_matting_grad_conn(ptr(pred_u8), ptr(target_u8), ptr(mask_u8), H, W,
                                                         self.acc_gc[self.frames].data_ptr(), None, self.ws.data_ptr(), st),
                         "matting_grad_conn")
        if self.flow_metrics and self.prev is not None:
            H, W = pred_u8.shape[-2:]
            if self.ws_fl_shape != (H, W):
                self.ws_fl = torch.empty(self.lib.otvm_optflow_farneback_ws_bytes(H, W), dtype=torch.uint8, device=pred_u8.device)
                self.ws_fl_shape = (H, W)
            # row i > 0: the pair (i-1, i), flow of (target i-1, target i)
            self.L.check(self.lib.otvm_matting_messddt(ptr(pp), ptr(tp), ptr(mp), ptr(pred_u8), ptr(target_u8), ptr(mask_u8), H, W,
                                                       self.acc_fl[self.frames].data_ptr(), None, self.ws_fl.data_ptr(), st),
                         "matting_messddt")
        self.prev = (pred_u8, target_u8, mask_u8)
        self.frames += 1

    def result(self):
        rows = self.acc[:self.frames].cpu()
        tot = rows.sum(0).tolist()
        sad_f = (rows[:, 0] / 255.0 / 1000.0).tolist()
        mse_f = (rows[:, 1] / 255.0 ** 2 / (rows[:, 2] + 1.0)).tolist()
        # row i > 0 holds the temporal term of the pair (i-1, i), masked by frame i-1's mask (metric.py:252-264)
        dt_f = (rows[1:, 3] / 255.0 ** 2).sqrt().tolist()
        dt_n = (rows[1:, 4] + 1.0).tolist()
        res = dict(frames=self.frames, sad_sum=tot[0] / 255.0 / 1000.0, mse_num=tot[1] / 255.0 ** 2, mask_sum=tot[2],
                   dt_err2_sum=tot[3] / 255.0 ** 2, dt_mask_sum=tot[4],
                   sad_mean=tot[0] / 255.0 / 1000.0 / max(1, self.frames),
                   sad_per_frame=sad_f, mse_per_frame=mse_f, dtssd_per_pair=dt_f, dtssd_num_per_pair=dt_n,
                   dtssd_sum=float(sum(dt_f)))
        if self.image_metrics:
            gc = self.acc_gc[:self.frames].cpu()
            res.update(grad_per_frame=gc[:, 0].tolist(), conn_per_frame=gc[:, 1].tolist(),
                       grad_sum=float(gc[:, 0].sum()), conn_sum=float(gc[:, 1].sum()),
                       ssda_per_frame=(rows[:, 1].sqrt() / 255.0).tolist(), ssda_num_per_frame=(rows[:, 2] + 1.0).tolist())
        if self.flow_metrics:
            fl = self.acc_fl[1:self.frames].cpu()
            fe = (fl[:, 0] / 255.0 ** 2).tolist()
            res.update(messddt_per_pair=fe, messddt_num_per_pair=(fl[:, 1] + 1.0).tolist(), messddt_sum=float(sum(fe)))
        return res


def sad(pred, ref, mask=None):
    """Sum of absolute differences / 1000 (reference utils/tmp/metric.py:177-182)."""
    d = (pred.float() - ref.float()).abs()
    if mask is not None:
        d = d * mask
    return float(d.sum()) / 1000.0
