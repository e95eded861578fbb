"""``run_video_matte``: the build-owned counterpart of the reference's per-sequence loop
(reference eval.py:157-228) -- frame flags, memory schedule, large-input rule, u8 quantisation.

BASELINE.json names a ``run_video_matte()`` call surface; the reference has no such function (its loop
is inlined in eval.py), so this reproduces that loop around the reference-shaped ``EvalModel``.
"""
import contextlib

import numpy as np
import torch

from . import guided, keys, temporal
from . import roi as _roi
from .alpha_model import background_colour
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


class _ClipPlan:
    """What run_video_matte does with a clip, decided before anything is uploaded (host only): every up-front refusal, in the order
    they have always been made, and the three routes as ONE description, so that the frame loop asks no "which route" question.
      steps      : (t, kind, first_frame, last_frame, memorize or None = memory_schedule's) in the order they are issued
      sources    : {frame: one-hot trimap | label map | Mask} of the trimap flow -- ``trimap`` is {0: trimap}, ``mask`` a Mask at
                   frame 0, ``masks`` a Mask on every frame -- or None: the alphas flow (a trimap derived from each frame's alpha)
      per_frame  : ``masks``: each source is made into a trimap at its own step and not kept; otherwise upload() makes them all,
                   once per clip
      keyed      : the caller gave ``keyframes``: the result carries anchor_frames and schedule
      natural    : the steps run in frame order (the metrics are fed as the frames come)
    The model is only asked for the band of a Mask that names none."""

    def __init__(self, model, frames, trimap, alphas, keyframes, mask, masks, backgrounds, work_scale, work_radius, work_eps, skip,
                 max_num, roi=None, roi_margin=32, key=None, frames_are_rgb=False):
        self.roi, self.region = None, None                # the checked (window or "auto", margin); run_video_matte's _RegionOfInterest
        self.key, self.frames, self.rereadable = None, None, False                # ``key``: the key and the source the pre-pass of roi="auto" reads again
        if key is not None:
            masks = self._keyed(key, frames, frames_are_rgb, roi, (("trimap", trimap), ("mask", mask), ("masks", masks),
                                                                   ("keyframes", keyframes), ("alphas", alphas),
                                                                   ("backgrounds", backgrounds)))
        if roi is not None:
            # (host only, like everything here: the window itself is placed by upload(), which has the sources on the device)
            self.roi = _RegionOfInterest.refuse(roi, roi_margin, frames, alphas, backgrounds, work_scale, masks)
        if work_scale is not None:
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
        T = len(frames)
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
        # (a plain sequence is checked before anything is uploaded; a streaming source is checked frame by frame in the loop)
        if (work_scale is not None and T > 0 and (isinstance(frames, (list, tuple, np.ndarray)) or torch.is_tensor(frames))
                and _as_tensor(frames[0]).dtype != torch.uint8):
            raise ValueError("run_video_matte: work_scale takes uint8 [H,W,3] frames (float frames have no working-resolution "
                             "route), got %s" % _as_tensor(frames[0]).dtype)
        self.keyed = keyframes is not None
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
        self.model, self.alphas, self.work_scale = model, alphas, work_scale
        self.per_frame = masks is not None
        self.sources = dict(enumerate(masks)) if self.per_frame else keyframes
        # every launch-stream write the preprocess reads is made once per clip (no per-frame alpha, no per-frame trimap)
        self.constant_inputs = keyframes is not None
        self.steps, self.kinds, self.k0, self.natural = [], {}, 0, True
        self.tri, self.lab, self.ones = {}, {}, None
        self.mask_hw = {}                                 # frame -> the size of the mask it was given (checked against the frame)
        self.T, self.skip, self.max_num = T, skip, max_num
        if self.roi is not None and self.sources is None:
            raise ValueError("run_video_matte: roi belongs to the trimap flow (`trimap`, `mask`, `keyframes` or `masks`): the window "
                             "is placed round the trimaps' classes")
        if T == 0:
            return
        for t, v in (self.sources or {}).items():
            if isinstance(v, Mask) and v.shape is not None:       # (a key's mask has its frame's size by construction)
                self.mask_hw[t] = v.shape
                if not self.per_frame:
                    v.band_for(model)                     # (as above: a missing band is refused before anything is uploaded)
        if self.per_frame:
            self.steps = [(i, "key", True, True, False) for i in range(T)]          # T clips of one frame: nothing to memorise
        elif keyframes is not None:
            self.kinds = {t: _keyframe_kind(v) for t, v in keyframes.items()}
            if "key" not in self.kinds.values():
                raise ValueError("run_video_matte: keyframes need at least one full trimap (one-hot [3,H,W])")
            self.k0 = min(t for t, k in self.kinds.items() if k == "key")
            # the schedule takes the effective skip: the large-input rule needs the resolution the model runs at, which the
            # trimaps carry
            h, w = np.shape(keyframes[self.k0])[-2:]
            if work_scale is not None:
                h, w = guided.work_size(h, w, work_scale)
            if self.roi is not None and isinstance(self.roi[0], tuple) and len(self.roi[0]) in (3, 4):
                h, w = self.roi[0][-2:]                   # (roi="auto" / "track": upload() sizes the window and schedules again)
            self._schedule(h, w)
        else:
            self.steps = [(i, "frame", i == 0, i == T - 1, None) for i in range(T)]  # alpha flow: eval.py's loop as it is
        self.natural = all(st[0] == j for j, st in enumerate(self.steps))

    def _keyed(self, key, frames, frames_are_rgb, roi, others):
        """``key``: every refusal that needs no frame, then one keys.KeyedMask per frame -- the ``masks`` the rest of the plan sees."""
        for name, other in others:
            if other is not None:
                raise ValueError("run_video_matte: `key` mattes every frame from the trimap of its own key and excludes `%s`" % name)
        self.key = keys.check_key(key)
        if _roi.track_spec(roi, "run_video_matte") is not None:
            raise ValueError("run_video_matte: roi='track' follows a PROPAGATED trimap; `key` mattes every frame from its own key, "
                             "and roi='auto' already tracks there")
        plain = isinstance(frames, (list, tuple, np.ndarray)) or torch.is_tensor(frames)
        self.rereadable = plain or bool(getattr(frames, "rereadable", False))
        if isinstance(roi, str) and roi == "auto" and not self.rereadable:
            raise ValueError("run_video_matte: `key` with roi='auto' reads every frame twice (a pre-pass takes the box of every "
                             "frame's unknown band), and this source can be read once; give a window roi=(y0, x0, h, w)")
        if plain and len(frames) > 0:
            f0 = _as_tensor(frames[0])
            self.check_keyed_frame(f0)
        self.frames = frames
        return [keys.KeyedMask(key, frames_are_rgb) for _ in range(len(frames))]

    def check_keyed_frame(self, f):
        """(a plain sequence: before anything is uploaded; a streaming source: frame by frame, in the loop)"""
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
            raise ValueError("run_video_matte: `key` takes uint8 [H,W,3] frames (float frames have no key route), got %s %s"
                             % (f.dtype, tuple(f.shape)))
        self.key.check_frames(int(f.shape[0]), int(f.shape[1]))

    def bind(self, i, frame):
        """``key``: frame ``i`` as it is staged on the device is what its key is taken from (nothing is uploaded for it)"""
        if self.key is not None:
            self.sources[i].bind(frame)

    def _schedule(self, h, w):
        """The keyframe steps of a clip the model runs at h x w (the large-input rule doubles the effective skip)."""
        large = memory_schedule(0, h, w, self.skip, self.max_num)[2]
        self.steps = keyframe_schedule(self.T, self.kinds, int(self.skip * 2) if large else self.skip)

    def _trimap(self, v, dev):
        """One source of kind "key" as the model takes it: [1,1,3,h,w] on the device, reduced to the working resolution."""
        if isinstance(v, Mask):
            v = v.convert(self.model, dev)
        t = _as_tensor(v).to(dev).float()
        if self.work_scale is not None:
            t = guided.downsample_trimap(t, self.work_scale)
        return t[None, None]

    def upload(self, dev):
        """The part that needs the device, once per clip at the resolution given: the user trimap (25 MB as fp32 at 1080p) is
        uploaded once, not once per frame.  (``masks`` converts per frame: inputs().)"""
        if self.sources is None or not self.steps:
            return
        if self.per_frame:
            if self.region is not None:
                self._track(dev)
            return
        # masks become ordinary trimaps / label maps here, all of them before anything is reduced
        plain = {t: v.convert(self.model, dev) if isinstance(v, Mask) else v for t, v in self.sources.items()}
        if self.region is not None:
            plain = self._window(plain, dev)
        for t, v in plain.items():
            if self.kinds[t] == "key":
                self.tri[t] = self._trimap(v, dev)
            else:
                self.lab[t] = _as_tensor(v).to(dev)
                if self.work_scale is not None:
                    self.lab[t] = guided.downsample_labels(self.lab[t], self.work_scale)

    def _track(self, dev):
        """``masks`` with ``roi``: the pre-pass.  Every mask is converted and the box of its unknown band taken -- T box calls into
        one [T,8] buffer, ONE read-back -- and the region places a window per frame.  No trimap is kept: inputs() converts again."""
        if self.key is not None:
            return self._track_keyed(dev)
        if len(set(self.mask_hw.values())) != 1:
            raise ValueError("run_video_matte: roi needs masks of one resolution, got %s" % sorted(set(self.mask_hw.values())))
        (H, W), = set(self.mask_hw.values())
        rows = torch.empty((self.T, 8), dtype=torch.int32, device=dev)
        for t in range(self.T):
            _roi.trimap_bbox(self.sources[t].convert(self.model, dev), rows[t])
        self.region.place_tracking(_roi.boxes_of(rows)[0], H, W)

    def _track_keyed(self, dev):
        """``key`` with ``roi``: the same pre-pass, with one extra upload of each frame -- its key is taken, converted and boxed; T box
        calls into one [T,8] buffer, ONE read-back.  Nothing is kept: the frame loop stages and keys every frame again.  A window
        given by the caller is held against every frame's band by the same pre-pass, as ``masks`` holds it, when the source can be
        read twice; a source that is read once cannot be, and there the window is taken as it is."""
        if self.region.spec != "auto" and not self.rereadable:
            return self.region.place_fixed(self.T)
        rows, HW = torch.empty((self.T, 8), dtype=torch.int32, device=dev), None
        for t in range(self.T):
            f = _as_tensor(self.frames[t])
            self.check_keyed_frame(f)
            if HW is not None and tuple(f.shape[:2]) != HW:
                raise ValueError("run_video_matte: roi needs frames of one resolution, got %dx%d and %dx%d" % (HW + tuple(f.shape[:2])))
            HW = tuple(f.shape[:2])
            ready = getattr(f, "_otvm_ready", None)
            if ready is not None:
                torch.cuda.current_stream(dev).wait_event(ready)
            self.sources[t].bind(f.to(dev, non_blocking=True))
            _roi.trimap_bbox(self.sources[t].convert(self.model, dev), rows[t])
            self.sources[t].bind(None)
        self.region.place_tracking(_roi.boxes_of(rows)[0], HW[0], HW[1])

    def _window(self, plain, dev):
        """``roi`` with sources that serve the whole clip: the region places ONE window from the union of their non-background
        boxes (label maps count with their labels 1 and 2; one [n,8] buffer, one read-back) and every source is cropped to it, once."""
        order = sorted(plain)
        on_dev = {t: _as_tensor(plain[t]).to(dev) for t in order}
        on_dev = {t: v.float() if self.kinds[t] == "key" else v for t, v in on_dev.items()}
        sizes = {tuple(v.shape[-2:]) for v in on_dev.values()}
        if len(sizes) != 1:
            raise ValueError("run_video_matte: roi needs trimaps / label maps of one resolution, got %s" % sorted(sizes))
        (H, W), = sizes
        rows = torch.empty((len(order), 8), dtype=torch.int32, device=dev)
        for j, t in enumerate(order):
            _roi.trimap_bbox(on_dev[t], rows[j])
        if self.region.follows:
            # the tracking window: the same read-back decides the SIZE only; the sources stay at H x W on the device and each is
            # cropped at its own step, where the window then is (region.stage fills self.tri / self.lab)
            self.region.place_track(on_dev, dict(zip(order, rows)), {t: r[4:] for t, r in zip(order, _roi.rows_of(rows))}, H, W, self.T)
            self._schedule(*self.region.size)
            return {}
        self.region.place_static(dict(zip(order, _roi.boxes_of(rows)[1])), H, W, self.T)
        win = self.region.window(0)
        self._schedule(win[2], win[3])
        return {t: (_roi.crop(win, trimap=v)[1] if self.kinds[t] == "key" else _roi.crop(win, labels=v)[2]) for t, v in on_dev.items()}

    def check_masks(self, i, full_hw):
        """The one refusal of the masks that needs a frame: masks of a keyframe clip are all held against the first frame that
        comes by, those of ``masks`` each against its own."""
        for t in ([i] if self.per_frame else list(self.mask_hw)):
            if t not in self.mask_hw:
                continue                                  # (``key``: the frame itself was checked when it was bound)
            hw = self.mask_hw.pop(t)
            if tuple(hw) != tuple(full_hw):
                raise ValueError("run_video_matte: the mask of frame %d is %dx%d, the frames are %dx%d (masks are given at "
                                 "the frames' resolution)" % (t, hw[0], hw[1], full_hw[0], full_hw[1]))

    def inputs(self, i, kind, first_frame, H, W, dev):
        """(a, tri_gt, further keywords) of the model call of step ``i`` at H x W."""
        if self.sources is None:
            return _as_tensor(self.alphas[i]).to(dev).float()[None, None, None], None, {}
        self.ones = _ones_alpha(self.ones, H, W, dev)
        if self.per_frame and self.region is not None:
            return self.ones, self.region.take_trimap()[None, None], {}   # (cropped with the frame, in stage()'s one launch)
        if self.per_frame:
            return self.ones, self._trimap(self.sources[i], dev), {}     # this frame's own trimap; nothing is kept of it
        more = {}
        if kind == "key" and not first_frame:
            more["keyframe"] = True
        elif kind == "labels":
            more["labels"] = self.lab[i]
        # (as eval.py does, every frame is handed a trimap -- it comes back as out[2]; only a keyframe consumes it)
        return self.ones, self.tri.get(i, self.tri[self.k0]), more


def _ones_alpha(held, H, W, dev):
    """The dummy alpha of the trimap flow: one tensor for the whole clip, made anew only when the size changes."""
    if held is None or held.shape[-2:] != (H, W):
        held = torch.ones(1, 1, 1, H, W, device=dev)
    return held


def _stage_frame(f, b, dev, frames_are_rgb):
    """Frame tensor ``f`` and its optional background ``b`` as the model takes them: (fg, bg, H, W, whether the model's
    ``_frames_rgb`` applies, f's upload event, b's upload event).  The events are those the IO pipeline's prefetcher hangs on what
    it uploads (``_otvm_ready``); NOTHING waits for them here -- when the launch stream does is the caller's decision."""
    if f.dtype == torch.uint8 and (b is None or b.dtype == torch.uint8):
        # decoded images go to the device as they are ([H,W,3] uint8): the preprocess kernel converts, flips the
        # channel order and composites -- no per-frame torch conversion / transposition kernels
        fg = f.to(dev, non_blocking=True)
        bg = fg if b is None else b.to(dev, non_blocking=True)
        return fg, bg, fg.shape[0], fg.shape[1], True, getattr(f, "_otvm_ready", None), getattr(b, "_otvm_ready", None)
    planar = []
    for x in (f, b):                                      # backgrounds come in the same channel order as the frames
        if x is not None:
            x = x.to(dev).float()
            if frames_are_rgb:
                x = x.flip(-1)
            x = x.permute(2, 0, 1)[None, None].contiguous()
        planar.append(x)
    fg, bg = planar[0], planar[0] if b is None else planar[1]
    return fg, bg, fg.shape[-2], fg.shape[-1], False, None, None


class _WorkingResolution:
    """``work_scale``'s side of a frame step: stage() reduces the frame for the network, finish() brings alpha (and F) back to
    H x W through the guided filter and makes the foreground bytes there."""

    def __init__(self, scale, radius, eps, foreground, frames_are_rgb, new_background):
        self.scale, self.radius, self.eps, self.foreground, self.rgb = scale, radius, eps, foreground, frames_are_rgb
        self.new_background, self.bg_cache = new_background, {}
        self.ups, self.full = None, None

    @property
    def size(self):
        return None if self.ups is None else (self.ups.h, self.ups.w)

    def stage(self, f, dev):
        """_stage_frame's tuple for the reduced frame.  Its upload event is waited for HERE: the reduction reads the upload on
        the launch stream, so no event is left for the caller."""
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
            raise ValueError("run_video_matte: work_scale takes uint8 [H,W,3] frames (float frames have no "
                             "working-resolution route), got %s %s" % (f.dtype, tuple(f.shape)))
        ready = getattr(f, "_otvm_ready", None)
        self.full = f.to(dev, non_blocking=True).contiguous()
        if ready is not None:
            torch.cuda.current_stream(dev).wait_event(ready)
        if self.ups is None or (self.ups.H, self.ups.W) != tuple(self.full.shape[:2]):
            self.ups = guided.GuidedUpsampler(dev, self.full.shape[0], self.full.shape[1], self.scale, self.radius, self.eps,
                                              4 if self.foreground else 1)
        fg = self.ups.reduce(self.full)
        return fg, fg, self.ups.h, self.ups.w, True, None, None

    def finish(self, i, fg, alpha, engine, dev, make_bytes=True):
        """(alpha, alpha_u8, rgba, comp) at H x W: guided upsampling on this stream, behind the frame; the guide is the working
        frame the network saw.  The composite is made here, at full resolution, not by the engine.  make_bytes=False leaves the
        foreground bytes to a later foreground_bytes() (the temporal stabilisation changes alpha first)."""
        alpha, u8, self.fgr_full = self.ups.upsample(self.full, fg, [alpha] + (list(engine.last_fgr) if self.foreground else []))
        if not (self.foreground and make_bytes):
            return alpha, u8, None, None
        return (alpha, u8) + self.foreground_bytes(i, alpha, dev)

    def foreground_bytes(self, i, alpha, dev):
        """(rgba, comp) of ``alpha`` and the frame's full-resolution F over frame ``i``'s new background"""
        nb = None if self.new_background is None else _background_at(self.new_background, i, dev, self.bg_cache)
        if isinstance(nb, tuple):
            background_colour(nb, "run_video_matte")
        return self.ups.foreground_bytes(alpha, self.fgr_full, self.rgb, nb)


class _RegionOfInterest:
    """``roi``'s side of a frame step: stage() crops the frame (with ``masks`` also the frame's trimap, in the same launch) to the
    frame's window, finish() pastes the window's alpha, trimap (and F) back into H x W.  refuse() is the host-only part, before
    anything is uploaded; the windows are placed by _ClipPlan.upload(), which holds the sources:
      place_tracking : ``masks``: one size for the clip (one engine plan), an origin per frame from the frame's unknown box;
                       outside the window alpha follows the frame's own trimap
      place_static   : every other route: one window for the clip; outside it is background, and nothing there is looked at
      place_track    : roi="track" on those routes: one size for the clip, an origin per frame that lives ON THE DEVICE (a row of an
                       int32 log, otvm_roi_track): a step with a trimap of its own centres on it, every other step follows the
                       box of the output trimap of its already-matted temporal neighbour (roi.track_origin), one frame behind.
                       Sources are cropped per step, with the frame; nothing is read back between the first and the last frame"""

    def __init__(self, plan, foreground, frames_are_rgb, new_background):
        self.spec, self.margin = plan.roi
        self.plan, self.foreground, self.rgb = plan, foreground, bool(frames_are_rgb)
        self.new_background, self.bg_cache = new_background, {}
        self.windows, self.HW, self.tracking = None, None, False
        self.full = self.outside = self.tri = self.fgr_full = None
        self.rows, self.seen = None, []                   # static: [T,8] boxes of the output trimaps, in window coordinates
        self.follows = isinstance(self.spec, tuple) and self.spec[0] == "track"     # place_track's mode
        self.track_size, self.log, self.sources, self.source_rows = None, None, {}, {}
        self.pending = 0                                  # place_fixed: the frames whose window waits for the first frame's size

    @staticmethod
    def refuse(spec, margin, frames, alphas, backgrounds, work_scale, masks=None):
        """-> (the window as four ints, "auto", or ("track",) / ("track", h, w); the margin)"""
        track = _roi.track_spec(spec, "run_video_matte")
        if track is not None:
            spec = track
            if masks is not None:
                raise ValueError("run_video_matte: roi='track' follows a PROPAGATED trimap; `masks` mattes every frame from its own "
                                 "mask, and roi='auto' already tracks there")
        elif isinstance(spec, str):
            if spec != "auto":
                raise ValueError("run_video_matte: roi is None, 'auto', 'track' or a window (y0, x0, h, w), got %r" % (spec,))
        else:
            try:
                ok = len(spec) == 4 and all(not isinstance(v, bool) and int(v) == v for v in spec)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("run_video_matte: roi is None, 'auto' or a window (y0, x0, h, w) of four integers, got %r" % (spec,))
            spec = tuple(int(v) for v in spec)
            if spec[0] < 0 or spec[1] < 0 or spec[2] < 1 or spec[3] < 1:
                raise ValueError("run_video_matte: the window roi = (y0, x0, h, w) needs y0, x0 >= 0 and h, w >= 1, got %r" % (spec,))
        margin = _roi.check_margin(margin, "run_video_matte")
        if alphas is not None:
            raise ValueError("run_video_matte: roi belongs to the trimap flow; the alphas flow (VideoMatting108: trimaps from "
                             "ground-truth alpha) has no region-of-interest route")
        if backgrounds is not None:
            raise ValueError("run_video_matte: roi takes no per-frame `backgrounds` (they belong to the alphas flow)")
        if work_scale is not None:
            raise ValueError("run_video_matte: roi and work_scale exclude each other (a window at the working resolution is out "
                             "of scope); give one of them")
        if len(frames) > 0 and (isinstance(frames, (list, tuple, np.ndarray)) or torch.is_tensor(frames)):
            f0 = _as_tensor(frames[0])
            if f0.dtype != torch.uint8:
                raise ValueError("run_video_matte: roi takes uint8 [H,W,3] frames (float frames have no region-of-interest "
                                 "route), got %s" % f0.dtype)
            if track and len(spec) == 3:
                _roi.check_size(spec[1:], f0.shape[0], f0.shape[1], "run_video_matte: roi")
            elif not track and not isinstance(spec, str):
                _roi.check_window(spec, f0.shape[0], f0.shape[1], "run_video_matte: roi")
        return spec, margin

    def place_tracking(self, unknown, H, W):
        self.HW, self.tracking = (H, W), True
        if self.spec == "auto":
            h, w = _roi.window_size(unknown, H, W, self.margin)
            self.windows, at = [], (0, 0)
            for box in unknown:
                at = _roi.window_origin(box, h, w, H, W, at)
                self.windows.append(at + (h, w))
            return
        win = _roi.check_window(self.spec, H, W, "run_video_matte: roi")
        for t, box in enumerate(unknown):
            if not _roi.contains(win, box):
                raise ValueError("run_video_matte: the window roi = %r does not hold the unknown band of frame %d's mask (rows "
                                 "%d ... %d, columns %d ... %d)" % (win, t, box[0], box[2], box[1], box[3]))
        self.windows = [win] * len(unknown)

    def place_fixed(self, T):
        """``key`` with a window given by the caller and a source that is read once: no pre-pass is possible, nothing is known of
        the frames yet.  The window is held against the first frame's size in stage(); it is NOT held
        against the frames' unknown bands, which only a read-back could tell: outside it alpha follows the frame's own trimap."""
        self.tracking, self.pending = True, T

    def place_static(self, nonbg, H, W, T):
        """nonbg: {frame: the non-background box of the source given for it}"""
        self.HW = (H, W)
        if self.spec == "auto":
            box = _roi.union(nonbg.values()) or (H, W, -1, -1)
            h, w = _roi.window_size([box], H, W, self.margin)
            win = _roi.window_origin(box, h, w, H, W) + (h, w)
        else:
            win = _roi.check_window(self.spec, H, W, "run_video_matte: roi")
            for t, box in sorted(nonbg.items()):
                if not _roi.contains(win, box):
                    raise ValueError("run_video_matte: the window roi = %r does not hold the trimap / label map of frame %d (its "
                                     "classes other than background: rows %d ... %d, columns %d ... %d)"
                                     % (win, t, box[0], box[2], box[1], box[3]))
        self.windows = [win] * T

    def place_track(self, sources, source_rows, nonbg, H, W, T):
        """sources: {frame: the trimap / label map at H x W on the device}; source_rows: {frame: its int32 [8] box row on the
        device}; nonbg: {frame: its non-background box on the host} -- which decides the SIZE, and only that"""
        self.HW, self.sources, self.source_rows = (H, W), sources, source_rows
        h, w = _roi.track_size(nonbg, self.spec, self.margin, H, W, "run_video_matte", "the trimap / label map of frame %d")
        self.track_size, self.hold = (h, w), _roi.hold_of(self.margin)
        self.log = _roi.new_log((T,), h, w, next(iter(source_rows.values())).device)

    def window(self, i):
        return self.windows[i]

    @property
    def size(self):
        if self.follows:
            return self.track_size
        return None if not self.windows else tuple(self.windows[0][2:])

    def stage(self, f, i, dev):
        """_stage_frame's tuple for frame ``i``'s window.  The upload event is waited for HERE: the crop reads the upload on the
        launch stream, so no event is left for the caller."""
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
            raise ValueError("run_video_matte: roi takes uint8 [H,W,3] frames (float frames have no region-of-interest "
                             "route), got %s %s" % (f.dtype, tuple(f.shape)))
        if self.HW is None and self.pending:
            self.HW = tuple(int(v) for v in f.shape[:2])
            self.windows = [_roi.check_window(self.spec, self.HW[0], self.HW[1], "run_video_matte: roi")] * self.pending
        if tuple(f.shape[:2]) != self.HW:
            raise ValueError("run_video_matte: frame %d is %dx%d, the trimaps the window was placed in are %dx%d"
                             % ((i,) + tuple(f.shape[:2]) + self.HW))
        ready = getattr(f, "_otvm_ready", None)
        self.full = f.to(dev, non_blocking=True).contiguous()
        if ready is not None:
            torch.cuda.current_stream(dev).wait_event(ready)
        self.plan.bind(i, self.full)
        if self.follows:
            return self._stage_track(i, dev)
        win = self.windows[i]
        if self.tracking:
            # this frame's own trimap, at H x W: what the paste shows outside the window; nothing of it outlives the step
            self.outside = self.plan.sources[i].convert(self.plan.model, dev)
            fg, self.tri, _ = _roi.crop(win, frame=self.full, trimap=self.outside)
        else:
            fg = _roi.crop(win, frame=self.full)[0]
        return fg, fg, win[2], win[3], True, None, None

    def _stage_track(self, i, dev):
        """The tracking window's stage: the launch that decides row ``i`` of the origin log, then ONE crop at that row of the
        frame and, in the same launch, of the step's trimap or label map (which _ClipPlan.inputs then finds cropped)."""
        plan, (H, W) = self.plan, self.HW
        kind = plan.kinds.get(i, "frame")
        if kind == "key":
            # a trimap of its own: centred on it (its box is in frame coordinates, there is no neighbour to start from)
            _roi.track(self.source_rows[i], None, self.log[i, 8:], self.track_size, H, W, self.hold)
        else:
            # the already-matted temporal neighbour on the side the sweep comes from (not the schedule's predecessor)
            n = i - 1 if i > plan.k0 else i + 1
            _roi.track(self.log[n, :8], self.log[n, 8:], self.log[i, 8:], self.track_size, H, W, self.hold)
        src = self.sources.get(i)
        fg, tri, lab = _roi.crop_at(self.log[i, 8:], self.track_size, frame=self.full, trimap=src if kind == "key" else None,
                                    labels=src if kind == "labels" else None)
        if kind == "key":
            plan.tri[i] = tri[None, None]
        elif kind == "labels":
            plan.lab[i] = lab
        return fg, fg, self.track_size[0], self.track_size[1], True, None, None

    def take_trimap(self):
        tri, self.tri = self.tri, None
        return tri

    def finish(self, i, out, engine, dev):
        """(alpha, alpha_u8, trimap) at H x W; with ``foreground`` the pasted F is kept for foreground_bytes().  A static window
        also files the box of the frame's output trimap, for roi_clipped."""
        tri = out[1][0, 0].contiguous()
        if self.follows:
            _roi.trimap_bbox(tri, self.log[i, :8])        # what the next frame's window follows, and roi_clipped's box
            self.seen.append(i)
            self.plan.lab.pop(i, None)
            alpha, u8, trimap, self.fgr_full = _roi.paste_at(
                self.log[i, 8:], self.track_size, self.HW[0], self.HW[1], out[3][0, 0, 0], tri,
                engine.last_fgr if self.foreground else None, self.full, self.rgb, None,
                ("alpha", "alpha_u8", "trimap") + (("fgr",) if self.foreground else ()))
            return alpha, u8, trimap
        if not self.tracking:
            if self.rows is None:
                self.rows = torch.empty((len(self.windows), 8), dtype=torch.int32, device=dev)
            _roi.trimap_bbox(tri, self.rows[i])
            self.seen.append(i)
        alpha, u8, trimap, self.fgr_full = _roi.paste(
            self.windows[i], self.HW[0], self.HW[1], out[3][0, 0, 0], tri, engine.last_fgr if self.foreground else None, self.full,
            self.rgb, self.outside, ("alpha", "alpha_u8", "trimap") + (("fgr",) if self.foreground else ()))
        self.outside = None
        return alpha, u8, trimap

    def foreground_bytes(self, i, alpha, dev):
        """(rgba, comp) at H x W of ``alpha`` and the pasted F over frame ``i``'s new background: otvm_fgr_outputs"""
        nb = None if self.new_background is None else _background_at(self.new_background, i, dev, self.bg_cache)
        if isinstance(nb, tuple):
            background_colour(nb, "run_video_matte")
        return guided.foreground_bytes(alpha, self.fgr_full, self.rgb, nb, "run_video_matte")

    def result(self):
        """roi, roi_size and roi_clipped (ONE read-back of the boxes, after the last frame)"""
        if self.follows:
            if self.log is None:
                return dict(roi=[], roi_size=None, roi_clipped=[])
            self.windows, clipped = _roi.clipped(_roi.rows_of(self.log), self.track_size, *self.HW, self.seen)
            return dict(roi=list(self.windows), roi_size=self.size, roi_clipped=clipped)
        clipped = []
        if self.rows is not None:
            assert all(win[2:] == self.size for win in self.windows)                 # place_static: ONE window for the clip
            rows = [boxes + win[:2] for boxes, win in zip(_roi.rows_of(self.rows), self.windows)]       # (the fixed origins)
            clipped = _roi.clipped(rows, self.size, *self.HW, self.seen)[1]
        return dict(roi=list(self.windows or []), roi_size=self.size, roi_clipped=clipped)


class _Stabilisation:
    """``stabilise``'s side of a frame step: the temporal filter of alpha (otvm_amd/temporal.py) behind the frame -- and behind
    _WorkingResolution.finish -- on the launch stream.  refuse() is the host-only part, before anything is uploaded."""

    def __init__(self, options, frames_are_rgb):
        self.options, self.rgb, self.filter = options, bool(frames_are_rgb), None

    @staticmethod
    def refuse(plan, frames, backgrounds):
        if backgrounds is not None:
            raise ValueError("run_video_matte: stabilise takes no per-frame `backgrounds`: the flow is taken between the frames "
                             "as they are staged, and with `backgrounds` the network mattes their composite, which is not staged")
        if not plan.natural:
            raise ValueError("run_video_matte: stabilise needs the frames in natural order (the filter is causal: each frame "
                             "leans on the one before it); this keyframe schedule sweeps backward from frame %d" % plan.k0)
        if (len(frames) > 0 and (isinstance(frames, (list, tuple, np.ndarray)) or torch.is_tensor(frames))
                and _as_tensor(frames[0]).dtype != torch.uint8):
            raise ValueError("run_video_matte: stabilise takes uint8 [H,W,3] frames (the flow is OpenCV's Farneback flow of the "
                             "8-bit grey frames; float frames have no such route), got %s" % _as_tensor(frames[0]).dtype)

    def check_frame(self, f):
        """(a streaming source is checked frame by frame)"""
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
            raise ValueError("run_video_matte: stabilise takes uint8 [H,W,3] frames (the flow is OpenCV's Farneback flow of the "
                             "8-bit grey frames; float frames have no such route), got %s %s" % (f.dtype, tuple(f.shape)))

    def step(self, frame, alpha, trimap, tri_scale, dev):
        """(stabilised alpha, its byte) of the frame staged on the device [H,W,3], its raw alpha [H,W] and the trimap the
        network put out [3,h,w]"""
        from .temporal import TemporalStabiliser
        H, W = alpha.shape
        if self.filter is None or (self.filter.H, self.filter.W) != (H, W):
            self.filter = TemporalStabiliser(dev, H, W, **self.options)
        return self.filter.step(frame, alpha, trimap=trimap, tri_scale=tri_scale, rgb=self.rgb)


class _Collector:
    """The outputs of one clip, placed by frame index (the steps may come in any order) and stacked at the end.  Everything is
    kept where it is with ``keep_on_device`` and brought to the host as it comes otherwise.  With ``on_foreground`` the foreground
    frames are handed over and none is kept."""

    def __init__(self, T, keep_on_device, foreground, composite, on_foreground=None, raw=False):
        self.keep = (lambda x: x) if keep_on_device else (lambda x: x.cpu())
        self.alpha, self.u8, self.trimap, self.bank, self.anchors = ([None] * T for _ in range(5))
        self.raw = [None] * T if raw else None            # ``stabilise``: the alpha before the temporal filter
        self.on_foreground = on_foreground if foreground else None
        self.rgba = [None] * T if foreground and on_foreground is None else None
        self.comp = [None] * T if self.rgba is not None and composite else None

    def log_bank(self, i, frames, anchors=()):
        """The frame ids resident after frame ``i``'s update, and those of them that are anchors (host lists)."""
        self.bank[i], self.anchors[i] = list(frames), list(anchors)

    def put(self, i, alpha, u8, trimap, rgba=None, comp=None, raw=None):
        self.alpha[i], self.u8[i], self.trimap[i] = self.keep(alpha), self.keep(u8), self.keep(trimap)
        if self.raw is not None:
            self.raw[i] = self.keep(raw)
        if self.on_foreground is not None:
            self.on_foreground(i, rgba, comp)
        if self.rgba is not None:
            self.rgba[i] = self.keep(rgba)
        if self.comp is not None:
            self.comp[i] = self.keep(comp)

    def result(self, metrics=None, schedule=None, work_size=None, roi=None):
        res = dict(alpha=torch.stack(self.alpha), alpha_u8=torch.stack(self.u8), trimap=torch.stack(self.trimap),
                   bank_frames=self.bank)
        if schedule is not None:
            res.update(anchor_frames=self.anchors, schedule=schedule)
        if work_size is not None:
            res["work_size"] = work_size
        if roi is not None:
            res.update(roi)
        if self.raw is not None:
            res["alpha_raw"] = torch.stack(self.raw)
        if self.rgba is not None:
            res["fgr_u8"] = torch.stack(self.rgba)
        if self.comp is not None:
            res["comp_u8"] = torch.stack(self.comp)
        if metrics is not None:
            res["metrics"] = metrics.result()
        return res


def run_video_matte(model, frames, trimap=None, alphas=None, backgrounds=None, skip=10, max_num=5,
                    frames_are_rgb=False, on_frame=None, device=None, keep_on_device=False, gt_alpha_u8=None,
                    gt_mask_u8=None, gt_mask=None, gt_image_metrics=False, gt_flow_metrics=False, foreground=False,
                    new_background=None, keyframes=None, work_scale=None, work_radius=2, work_eps=1e-4, on_foreground=None,
                    mask=None, masks=None, stabilise=None, roi=None, roi_margin=32, key=None):
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
    stabilise   : None (off: a frame issues exactly the launches it issues without the option), True, a strength in [0,1], or a
                  dict of temporal.TemporalStabiliser's keywords (strength, tau_colour, tau_alpha, region): temporal
                  stabilisation of alpha, a causal flow-compensated recursive filter on the launch stream behind each frame
                  (and behind the guided upsampling of ``work_scale``, at H x W).  The previous stabilised alpha is fetched where
                  the Farneback flow of the grey frames points and blended in where the colours agree, alpha has not really
                  changed and -- region="unknown" -- the frame's trimap says unknown.  alpha, alpha_u8, on_frame's alpha / u8 and
                  the metrics carry the stabilised values, the result gains alpha_raw [T,H,W] (the alpha before the filter), and
                  with ``foreground`` / ``new_background`` the bytes are remade from the stabilised alpha and the frame's F
                  (fgr_u8[..., 3] == alpha_u8).  There is no trained checkpoint here: the filter is checked by definition and by
                  property on synthetic clips, not by quality on real footage, and the default parameters are PLACEHOLDERS.
                  Refused for float frames, with ``backgrounds`` and for a keyframe schedule that is not in natural order (a
                  backward sweep); not available in run_video_matte_batch.
    roi         : None (off: a frame issues exactly the launches it issues without the option), "auto", a window (y0, x0, h, w),
                  "track" or ("track", h, w):
                  region-of-interest matting.  Every frame (uint8 [H,W,3] only) is cropped on the device to an h x w window, the
                  network runs there -- the memory schedule, large-input rule included, is evaluated at h x w -- and alpha, the
                  trimap (with ``foreground`` also F) are pasted back into H x W (otvm_amd/roi.py).  Checked BY DEFINITION ONLY:
                  the result is, bit for bit, the matte of the cropped clip pasted back.  It is NOT the full-frame result -- the
                  decoder's pyramid pooling sees the window, not the frame -- and with no trained checkpoint here nobody can say
                  how the two compare on real footage.  "auto" with ``masks`` TRACKS: a pre-pass converts every mask and takes the
                  box of its unknown band (one read-back), the largest box plus ``roi_margin`` on every side, rounded up to a
                  multiple of 32, is the clip's one window size, and each frame's window is centred on its own box; outside the
                  window alpha is 1 / 0 by the frame's own trimap, and the window holds the whole unknown band by construction.
                  "auto" with ``trimap`` / ``mask`` / ``keyframes`` places ONE window for the clip round the classes other than
                  background of all the sources (label maps count with their labels 1 and 2); everything outside it is
                  background and is never looked at, so the subject must STAY inside: the result's roi_clipped lists the frames
                  whose propagated trimap reaches a side of the window that is not a side of the frame.  A window given by the
                  caller serves every frame of any route and is refused when a source does not fit in it (``masks``: the unknown
                  band of any frame).  alpha, alpha_u8, trimap, fgr_u8, comp_u8, alpha_raw, on_frame's alpha / u8 and the metrics
                  are at H x W (on_frame's ``out`` is the network's, at h x w); the foreground bytes are made at full resolution
                  from the pasted planes, ``stabilise`` runs behind the paste.  The result gains roi=[(y0, x0, h, w) per frame],
                  roi_size=(h, w) and roi_clipped.  Every window size is an engine plan of its own and NOTHING is evicted here: a
                  process that mattes many clips drops them itself (EvalModel.drop_plans).  Refused for float frames, the
                  ``alphas`` flow, ``backgrounds`` and together with ``work_scale``; not available in run_video_matte_batch.
                  "track" or ("track", h, w) with ``trimap`` / ``mask`` / ``keyframes``: the TRACKING window.  One size for the
                  clip (one engine plan) -- h x w as given, refused when a source's classes other than background do not fit; or
                  the largest source's box (not the union) plus ``roi_margin`` on every side, rounded up to a multiple of 32 -- and
                  an origin per frame that lives ON THE DEVICE (a row of an int32 log; otvm_roi_track): a step with a trimap of its
                  own (the first frame, full keyframes) is centred on it, every other step starts from its already-matted
                  temporal neighbour (t-1 in the forward sweep, t+1 in the backward one) and, per axis, HOLDS that origin while
                  the non-background box of the trimap returned for that frame keeps hold = max(1, roi_margin // 2) pixels from
                  both window sides (a side that is the frame's counts as held), and recentres on the box otherwise
                  (roi.track_origin).  Nothing is read back inside the frame loop: the sources' boxes once before the first frame,
                  the origins and the output boxes once after the last.  The window LAGS ONE FRAME: a subject that moves more than
                  ``hold`` pixels a frame, or outgrows the size, is cut -- roi_clipped lists those frames.  Outside the window
                  everything is background.  Checked by definition only, as above; refused with ``masks`` ("auto" tracks there).
    key         : a keys.ChromaKey (footage shot against a green / blue screen) or a keys.PlateKey (a locked-off shot with a clean
                  plate of the empty set): TRIMAP-FREE matting.  The mask of every frame is made on the device from the frame itself,
                  as it is already staged there (otvm_mask_from_chroma / otvm_mask_from_plate: no second upload, nothing read back
                  in the frame loop), made into a trimap as ``masks`` does, and the frame is matted from it: the ``masks`` route
                  unchanged -- each step a clip of one frame, natural order, bank_frames [] for every frame -- so ``frames`` may be
                  a source that is read once (a Y4MFrames on a pipe).  on_frame, the metrics, foreground / new_background /
                  on_foreground, work_scale (key and band at H x W, the trimap reduced as any other), stabilise and roi (a window,
                  or "auto") work as with ``masks``; roi="auto" needs the pre-pass over all frames (one extra upload of each, one
                  read-back of T boxes) and is refused for a source that cannot be read twice (a plain sequence can; any other
                  source says so with ``rereadable = True``); a window given by the caller is held against every frame's unknown
                  band by the same pre-pass and refused when one does not fit, as with ``masks`` -- except for a source that is read
                  once, where no pre-pass is possible: there it is taken as it is, held against the frames' size only (outside it
                  alpha follows the frame's own trimap; whether the band fits is then the caller's knowledge).  Exclusive with trimap, mask, masks, keyframes, alphas and
                  backgrounds; refused with roi="track", for float frames and for a plate of another size than the frames; not
                  available in run_video_matte_batch and run_video_matte_subjects.  To key only the first frame and propagate:
                  mask=Mask(keys.key_mask(f0, key).cpu()).  The keys are CHECKED BY DEFINITION ONLY (bit for bit against their
                  restatement) and every default of theirs is a PLACEHOLDER nobody tuned on real footage; with no trained
                  checkpoint here nothing is claimed about matting quality.
    roi_margin  : pixels kept round the box on every side by roi="auto" / "track", and twice the pixels a tracked box keeps from a
                  window side before the window moves (default 32: a PLACEHOLDER nobody tuned on real footage)
    Returns dict(alpha=[T,H,W] float32, alpha_u8=[T,H,W] uint8 (truncated, eval.py:209), trimap=[T,3,H,W],
    bank_frames=[per frame: ids of the frames resident in the memory bank after that frame's update]) and, when ``keyframes``
    was given, anchor_frames=[per frame: those of them that are anchors], schedule=[the steps issued, keyframe_schedule's tuples].
    """
    frames = list(frames) if not (hasattr(frames, "shape") or hasattr(frames, "__getitem__")) else frames
    T = len(frames)
    dev = device or next(model.parameters()).device
    plan = _ClipPlan(model, frames, trimap, alphas, keyframes, mask, masks, backgrounds, work_scale, work_radius, work_eps, skip,
                     max_num, roi, roi_margin, key, frames_are_rgb)
    stab = temporal.options_of(stabilise)
    if stab is not None:
        _Stabilisation.refuse(plan, frames, backgrounds)
        stab = _Stabilisation(stab, frames_are_rgb)
    core = model.module if hasattr(model, "module") else model
    foreground = bool(foreground) or new_background is not None
    work = (None if work_scale is None else
            _WorkingResolution(work_scale, work_radius, work_eps, foreground, frames_are_rgb, new_background))
    region = plan.region = None if plan.roi is None else _RegionOfInterest(plan, foreground, frames_are_rgb, new_background)
    col = _Collector(T, keep_on_device, foreground, new_background is not None, on_foreground, raw=stab is not None)
    metrics = (ClipMetrics(dev, image_metrics=gt_image_metrics, flow_metrics=gt_flow_metrics) if gt_alpha_u8 is not None
               else None)
    plan.upload(dev)
    bg_cache = {}
    with _foreground_option(core, foreground):
        for i, kind, first_frame, last_frame, step_memorize in plan.steps:
            f = _as_tensor(frames[i])
            b = _as_tensor(backgrounds[i]) if backgrounds is not None else None
            if stab is not None:
                stab.check_frame(f)
            if plan.key is not None:
                plan.check_keyed_frame(f)
            fg, bg, H, W, rgb_applies, ready, ready_b = (work.stage(f, dev) if work is not None else
                                                         region.stage(f, i, dev) if region is not None else
                                                         _stage_frame(f, b, dev, frames_are_rgb))
            extra = {"_frames_rgb": bool(frames_are_rgb)} if rgb_applies else {}
            if ready_b is not None:
                torch.cuda.current_stream(dev).wait_event(ready_b)
            if ready is not None:
                # the upload event may only travel to the model (whose query-encoder stream then starts on it, ahead of the
                # launch stream) when EVERYTHING the preprocess reads is covered by it or loop-invariant: the frame itself
                # (no copy made here), no separately uploaded background, and the trimap flow's constant alpha -- a per-frame
                # alpha or trimap is written by the launch stream just below.  Otherwise the launch stream waits for the upload
                # and the model orders its side streams behind the launch stream.
                if b is None and fg is f and plan.constant_inputs:
                    extra["_inputs_ready"] = ready
                else:
                    torch.cuda.current_stream(dev).wait_event(ready)
            plan.check_masks(i, work.full.shape[:2] if work is not None else region.HW if region is not None else (H, W))
            if plan.key is not None and region is None:
                plan.bind(i, fg if work is None else work.full)   # (roi: bound by region.stage, which converts there)
            a, tri_gt, more = plan.inputs(i, kind, first_frame, H, W, dev)
            plan.bind(i, None)
            if i == plan.k0 - 1:
                core.drop_non_anchors()                           # the backward sweep starts from the keyframes alone
            memorize, max_memory_num, large = memory_schedule(i, H, W, skip, max_num)
            if step_memorize is not None:
                memorize = step_memorize
            if foreground:
                # (working resolution: the composite is made at full resolution by work.finish, not by the engine)
                # (stabilise: made behind the temporal filter, from the stabilised alpha)
                # (roi: made behind the paste, at full resolution, by region.foreground_bytes)
                core.set_background(None if new_background is None or work is not None or stab is not None or region is not None
                                    else _background_at(new_background, i, dev, bg_cache))
            out = model(a, fg, bg, tri=None, tri_gt=tri_gt, first_frame=first_frame, last_frame=last_frame,
                        memorize=memorize, max_memory_num=max_memory_num, large_input=large, _frame_id=i, **extra, **more)
            alpha, u8, rgba, comp, tri_out = out[3][0, 0, 0], core._engine.last_alpha_u8, None, None, out[1][0, 0]
            if region is not None:
                alpha, u8, tri_out = region.finish(i, out, core._engine, dev)
                if foreground and stab is None:
                    rgba, comp = region.foreground_bytes(i, alpha, dev)
            elif work is not None:
                alpha, u8, rgba, comp = work.finish(i, fg, alpha, core._engine, dev, make_bytes=stab is None)
            elif foreground:
                rgba, comp = core._engine.last_rgba_u8, core._engine.last_comp_u8
            raw = None
            if stab is not None:
                # the frame as it was staged (its upload is behind the launch stream: the model waited for it), the alpha at
                # H x W and the trimap the network put out, at the resolution it ran at
                raw = alpha
                full = region.full if region is not None else fg if work is None else work.full
                alpha, u8 = stab.step(full, alpha, tri_out, 1 if work is None else work_scale, dev)
                if region is not None and foreground:
                    rgba, comp = region.foreground_bytes(i, alpha, dev)
                elif work is not None and foreground:
                    rgba, comp = work.foreground_bytes(i, alpha, dev)
                elif foreground:
                    nb = None if new_background is None else _background_at(new_background, i, dev, bg_cache)
                    if isinstance(nb, tuple):
                        background_colour(nb, "run_video_matte")
                    rgba, comp = guided.foreground_bytes(alpha, core._engine.last_fgr, frames_are_rgb, nb, "run_video_matte")
            mem_now = core.memories
            col.log_bank(i, mem_now["frames"], mem_now["anchors"])
            if metrics is not None and plan.natural:
                _metrics_add(metrics, u8, i, gt_alpha_u8, gt_mask_u8, gt_mask, dev)
            if on_frame is not None:
                on_frame(i, alpha, u8, out)
            col.put(i, alpha, u8, tri_out, rgba, comp, raw=raw)
    if metrics is not None and not plan.natural:
        # the pair terms (dtSSD, MESSDdt) depend on the order: fed in natural frame order from the kept 8-bit alphas
        for i in range(T):
            _metrics_add(metrics, col.u8[i].to(dev), i, gt_alpha_u8, gt_mask_u8, gt_mask, dev)
    return col.result(metrics, list(plan.steps) if plan.keyed else None, None if work is None else work.size,
                      None if region is None else region.result())


def _metrics_add(metrics, u8, i, gt_alpha_u8, gt_mask_u8, gt_mask, dev):
    g = _as_tensor(gt_alpha_u8[i])
    mk = gt_mask
    if gt_mask_u8 is not None:
        mk = _as_tensor(gt_mask_u8[i]).to(dev)
    metrics.add(u8, g.to(dev), mk)


def run_video_matte_batch(model, clips, trimaps=None, alphas=None, backgrounds=None, skip=10, max_num=5, frames_are_rgb=False,
                          device=None, keep_on_device=False, on_frame=None, gt_alpha_u8=None, gt_mask=None,
                          gt_image_metrics=False, gt_flow_metrics=False, foreground=False, new_background=None, keyframes=None,
                          work_scale=None, mask=None, masks=None, roi=None, key=None):
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
    if key is not None:
        raise ValueError("run_video_matte_batch: key (trimap-free matting of keyed footage) is a single-clip feature "
                         "(run_video_matte); lock-step batches take trimaps")
    if roi is not None:
        raise ValueError("run_video_matte_batch: roi (region-of-interest matting) is a single-clip feature (run_video_matte); the "
                         "clips of a lock-step batch share one resolution, a window per clip would not")
    B = len(clips)
    lens = [len(c) for c in clips]
    T = max(lens)
    if (trimaps is None) == (alphas is None):
        raise ValueError("run_video_matte_batch: give either trimaps (demo flow) or alphas (VideoMatting108 flow)")
    core = model.module if hasattr(model, "module") else model
    dev = device or next(core.parameters()).device
    foreground = bool(foreground) or new_background is not None
    if new_background is not None and not (isinstance(new_background, list) and len(new_background) == B):
        raise ValueError("run_video_matte_batch: new_background is a list of one entry per clip")
    cols = [_Collector(n, keep_on_device, foreground, new_background is not None) for n in lens]
    bg_cache = [{} for _ in range(B)]
    metrics = ([ClipMetrics(dev, image_metrics=gt_image_metrics, flow_metrics=gt_flow_metrics) for _ in range(B)]
               if gt_alpha_u8 is not None else [None] * B)
    tri_dev = [None] * B if trimaps is None else [_as_tensor(t).to(dev).float()[None, None] for t in trimaps]
    ones = None
    with _foreground_option(core, foreground):
        for i in range(T):
            A, FG, BG = [], [], []
            for b in range(B):
                j = min(i, lens[b] - 1)                               # a clip that has ended repeats its last frame (discarded)
                f = _as_tensor(clips[b][j])
                bk = _as_tensor(backgrounds[b][j]) if backgrounds is not None else None
                fg, bg, H, W, rgb_applies, *events = _stage_frame(f, bk, dev, frames_are_rgb)
                # frames handed over by the IO pipeline's prefetcher carry their upload event: the launch stream waits for
                # it before anything reads them (the batched step makes no promise to the engine about its inputs, so its
                # side streams order themselves behind the launch stream)
                for ev in events:
                    if ev is not None:
                        torch.cuda.current_stream(dev).wait_event(ev)
                if trimaps is not None:
                    a = ones = _ones_alpha(ones, H, W, dev)
                else:
                    a = _as_tensor(alphas[b][j]).to(dev).float()[None, None, None]
                A.append(a), FG.append(fg), BG.append(bg)
            memorize, max_memory_num, large = memory_schedule(i, H, W, skip, max_num)
            if foreground:
                core.set_background(None if new_background is None else
                                    [_background_at(new_background[b], min(i, lens[b] - 1), dev, bg_cache[b]) for b in range(B)])
            outs = core.forward_batch(A, FG, BG, tri_dev, first_frame=(i == 0), last_frame=(i == T - 1), memorize=memorize,
                                      max_memory_num=max_memory_num, large_input=large,
                                      _frames_rgb=rgb_applies and bool(frames_are_rgb))
            eng, bank = core._engine, core.memories["frames"]              # (one look at the bank per step)
            for b in range(B):
                if i >= lens[b]:
                    continue
                u8 = eng.last_alpha_u8_b[b]
                cols[b].log_bank(i, bank)
                if metrics[b] is not None:
                    _metrics_add(metrics[b], u8, i, gt_alpha_u8[b], None, gt_mask, dev)
                if on_frame is not None:
                    on_frame(b, i, outs[b][3][0, 0, 0], u8, outs[b])
                cols[b].put(i, outs[b][3][0, 0, 0], u8, outs[b][1][0, 0], eng.last_rgba_u8_b[b] if foreground else None,
                            eng.last_comp_u8_b[b] if new_background is not None else None)
    return [col.result(m) for col, m in zip(cols, metrics)]


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
