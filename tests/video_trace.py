"""What otvm_amd/video.py does around the model, observed on the CPU: a stub stands where the model does, everything that would
touch the device library is a recorder, and each case leaves the ordered list of what the driver did -- frame reads, event waits,
backgrounds set, conversions and reductions, every model call with every keyword, metrics, callbacks -- and what it returned.
tests/golden/video_driver_trace.json holds these traces as the driver gave them BEFORE it was restructured
(tests/golden/make_video_trace.py); tests/test_video_driver_cpu.py asserts that it still gives exactly them.

Tensors are recorded as dtype, shape and a checksum of their bytes; the stub's outputs are integer patterns derived from the frame
index, so every figure is exact."""
import hashlib

import numpy as np
import torch
from torch import nn

H, W = 6, 8


class Event:
    """An upload event: a sentinel hung on a frame tensor as ``_otvm_ready``."""

    def __init__(self, name):
        self.name = name


def digest(t):
    return hashlib.sha1(t.detach().contiguous().numpy().tobytes()).hexdigest()[:16]


def desc(x):
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, Event):
        return "event " + x.name
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if torch.is_tensor(x):
        return [str(x.dtype).replace("torch.", ""), list(x.shape), digest(x)]
    if isinstance(x, (list, tuple)):
        return [desc(v) for v in x]
    if isinstance(x, dict):
        return {str(k): desc(v) for k, v in x.items()}
    raise TypeError("video_trace: cannot record %r" % type(x))


class Trace:
    def __init__(self):
        self.events = []
        self.handed = []              # the frame objects the caller's sequences handed out

    def ev(self, *items):
        self.events.append([desc(i) for i in items])


class Seq:
    """A streaming source: len() and [i], each read recorded."""

    def __init__(self, tr, what, items):
        self.tr, self.what, self.items = tr, what, list(items)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        self.tr.ev("read", self.what, int(i))
        self.tr.handed.append(self.items[i])
        return self.items[i]


class ListSeq(list):
    """A plain list whose reads are recorded (the driver treats it as the plain sequence it is)."""

    def __init__(self, tr, what, items):
        super().__init__(items)
        self.tr, self.what = tr, what

    def __getitem__(self, i):
        self.tr.ev("read", self.what, int(i))
        x = super().__getitem__(i)
        self.tr.handed.append(x)
        return x


def pattern(seed, shape, dtype=torch.uint8):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.int64) * 7 + int(seed)) % 256).to(dtype).reshape(shape)


def _background_kind(bg):
    if bg is None:
        return "none"
    if isinstance(bg, tuple):
        return ["colour"] + [int(c) for c in bg]
    return ["image", desc(bg)]


def _background_term(bg):
    if bg is None:
        return None
    if isinstance(bg, tuple):
        return torch.tensor([int(c) % 256 for c in bg], dtype=torch.uint8)
    return bg


class _Engine:
    last_alpha_u8 = last_fgr = last_rgba_u8 = last_comp_u8 = None
    last_alpha_u8_b = last_rgba_u8_b = last_comp_u8_b = None


class StubModel(nn.Module):
    def __init__(self, tr):
        super().__init__()
        self.p = nn.Parameter(torch.zeros(1))
        self.DILATION_KERNEL = 3
        self.foreground, self._background = False, None
        self._engine = _Engine()
        self.tr = tr
        self.bank, self.anchors = [], []
        self.last_a, self.last_bg, self.step = None, None, 0

    @property
    def memories(self):
        return {"frames": self.bank, "anchors": self.anchors}

    def drop_non_anchors(self):
        self.tr.ev("drop_non_anchors")
        self.bank = list(self.anchors)

    def set_background(self, bg):
        now = bg if isinstance(bg, list) else [bg]
        was = self.last_bg if self.last_bg is not None else [object()] * len(now)
        self.tr.ev("set_background", [_background_kind(x) for x in now],
                   [torch.is_tensor(x) and any(x is y for y in was) for x in now])
        self.last_bg = now
        self._background = bg

    def _size(self, fg):
        return tuple(fg.shape[:2]) if fg.dtype == torch.uint8 and fg.dim() == 3 else tuple(fg.shape[-2:])

    def _outputs(self, seed, fg, tri_gt, background):
        h, w = self._size(fg)
        u8 = pattern(seed, (h, w))
        alpha = (u8.float() / 255)[None, None, None]
        tri = tri_gt if tri_gt is not None else pattern(seed + 1, (1, 1, 3, h, w), torch.float32)
        fgr = rgba = comp = None
        if self.foreground:
            fgr = [pattern(seed + 2 + c, (h, w)).float() / 255 for c in range(3)]
            rgba = pattern(seed + 5, (h, w, 4))
            term = _background_term(background)
            comp = None if term is None else pattern(seed + 6, (h, w, 3)) + term
        return (None, tri, None, alpha, None), u8, fgr, rgba, comp

    def _call(self, a, fg, bg, tri_gt):
        d = dict(a=desc(a), a_is_last_a=a is self.last_a, fg=desc(fg), bg_is_fg=bg is fg, fg_is_callers=any(fg is x for x in self.tr.handed),
                 tri_gt=desc(tri_gt))
        if bg is not fg:
            d["bg"] = desc(bg)
        self.last_a = a
        return d

    def forward(self, a, fg, bg, tri=None, tri_gt=None, first_frame=False, last_frame=False, memorize=False, max_memory_num=2,
                large_input=False, _frame_id=None, **extra):
        d = self._call(a, fg, bg, tri_gt)
        d.update(tri=tri, first_frame=first_frame, last_frame=last_frame, memorize=memorize, max_memory_num=max_memory_num,
                 large_input=large_input, _frame_id=_frame_id, foreground=self.foreground,
                 extra={k: extra[k] for k in sorted(extra)})
        self.tr.ev("model", d)
        if first_frame:
            self.bank, self.anchors = [], []
        if memorize:
            self.bank = self.bank + [_frame_id]
            if first_frame or extra.get("keyframe"):
                self.anchors = self.anchors + [_frame_id]
        eng = self._engine
        out, eng.last_alpha_u8, eng.last_fgr, eng.last_rgba_u8, eng.last_comp_u8 = self._outputs(_frame_id * 37, fg, tri_gt,
                                                                                                 self._background)
        return out

    def forward_batch(self, a, fg, bg, tri_gt, first_frame=False, last_frame=False, memorize=False, max_memory_num=2,
                      large_input=False, **extra):
        calls = [self._call(a[b], fg[b], bg[b], tri_gt[b]) for b in range(len(a))]
        self.tr.ev("model_batch", dict(clips=calls, first_frame=first_frame, last_frame=last_frame, memorize=memorize,
                                       max_memory_num=max_memory_num, large_input=large_input, foreground=self.foreground,
                                       extra={k: extra[k] for k in sorted(extra)}))
        if first_frame:
            self.bank, self.step = [], 0
        if memorize:
            self.bank = self.bank + [self.step]
        backgrounds = self._background if isinstance(self._background, list) else [self._background] * len(a)
        res = [self._outputs(self.step * 37 + b * 11, fg[b], tri_gt[b], backgrounds[b]) for b in range(len(a))]
        eng = self._engine
        eng.last_alpha_u8_b, eng.last_rgba_u8_b, eng.last_comp_u8_b = [r[1] for r in res], [r[3] for r in res], [r[4] for r in res]
        self.step += 1
        return [r[0] for r in res]


def install(monkeypatch, tr):
    """Recorders in place of everything of otvm_amd/video.py's that would touch the device library."""
    from otvm_amd import guided, video
    from otvm_amd.masks import Mask

    class Stream:
        def wait_event(self, e):
            tr.ev("wait_event", e)

    def convert(self, model, device):
        tr.ev("convert", self.role, self.data, self.band_for(model))
        d = torch.as_tensor(self.data)
        d = d.float() * 255 if d.dtype.is_floating_point else d.float()
        if self.role == "labels":
            return torch.where(d >= self.hi, 2, torch.where(d <= self.lo, 0, 255)).to(torch.uint8)
        return torch.stack([d <= self.lo, (d > self.lo) & (d < self.hi), d >= self.hi]).float()

    def downsample_trimap(tri, scale):
        tr.ev("downsample_trimap", tri, scale)
        return tri[:, ::scale, ::scale].contiguous()

    def downsample_labels(labels, scale):
        tr.ev("downsample_labels", labels, scale)
        return labels[::scale, ::scale].contiguous()

    class Upsampler:
        def __init__(self, device, H, W, scale, radius=2, eps=1e-4, channels=1):
            tr.ev("GuidedUpsampler", str(device), H, W, scale, radius, eps, channels)
            self.H, self.W, self.scale = H, W, scale
            self.h, self.w = guided.work_size(H, W, scale)

        def reduce(self, frame):
            tr.ev("reduce", frame, any(frame is x for x in tr.handed))
            return frame[::self.scale, ::self.scale].contiguous()

        def _up(self, t):
            return t.repeat_interleave(self.scale, 0).repeat_interleave(self.scale, 1)[:self.H, :self.W].contiguous()

        def upsample(self, frame, work_frame, targets):
            tr.ev("upsample", frame, work_frame, list(targets))
            alpha = self._up(targets[0])
            return alpha, (alpha * 255 + 0.5).to(torch.uint8), (torch.stack([self._up(t) for t in targets[1:]]) if len(targets) == 4
                                                                 else None)

        def foreground_bytes(self, alpha, fgr, rgb, background=None):
            tr.ev("foreground_bytes", alpha, fgr, rgb, _background_kind(background))
            rgba = torch.cat([(fgr.permute(1, 2, 0) * 255 + 0.5).to(torch.uint8), (alpha * 255 + 0.5).to(torch.uint8)[..., None]], -1)
            term = _background_term(background)
            return rgba, None if term is None else rgba[..., :3] + term

    class Metrics:
        def __init__(self, device, image_metrics=False, flow_metrics=False):
            tr.ev("ClipMetrics", str(device), image_metrics, flow_metrics)
            self.n = 0

        def add(self, pred_u8, target_u8, mask_u8=None):
            tr.ev("metrics_add", pred_u8, target_u8, mask_u8)
            self.n += 1

        def result(self):
            return {"frames": self.n}

    monkeypatch.setattr(Mask, "convert", convert)
    monkeypatch.setattr(guided, "GuidedUpsampler", Upsampler)
    monkeypatch.setattr(guided, "downsample_trimap", downsample_trimap)
    monkeypatch.setattr(guided, "downsample_labels", downsample_labels)
    monkeypatch.setattr(video, "ClipMetrics", Metrics)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream())


# -- inputs

def u8_frames(seed, T, h=H, w=W):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(T)]


def float_frames(seed, T):
    rs = np.random.RandomState(seed)
    return [rs.rand(H, W, 3).astype(np.float32) for _ in range(T)]


def with_events(arrays, prefix):
    out = []
    for i, a in enumerate(arrays):
        t = torch.from_numpy(a)
        t._otvm_ready = Event("%s%d" % (prefix, i))
        out.append(t)
    return out


def trimap(seed, h=H, w=W):
    cls = np.random.RandomState(seed).randint(0, 3, (h, w))
    return np.stack([cls == c for c in range(3)]).astype(np.float32)


def labels(seed, h=H, w=W):
    return np.random.RandomState(seed).choice(np.array([0, 1, 2, 255], np.uint8), (h, w))


def plane_u8(seed, T, h=H, w=W):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(T)]


def alphas(seed, T):
    return [a.astype(np.float32) / 255 for a in plane_u8(seed, T)]


def callbacks(tr):
    return dict(on_frame=lambda i, alpha, u8, out: tr.ev("on_frame", i, alpha, u8, out[1]),
                on_foreground=lambda i, rgba, comp: tr.ev("on_foreground", i, rgba, comp))


# -- the cases: name -> callable(tr, model) returning what the driver returned

def _single(tr, model, frames, wrap=Seq, **kw):
    from otvm_amd.video import run_video_matte
    if "backgrounds" in kw:
        kw["backgrounds"] = Seq(tr, "background", kw["backgrounds"])
    if "alphas" in kw:
        kw["alphas"] = Seq(tr, "alpha", kw["alphas"])
    kw.setdefault("on_frame", callbacks(tr)["on_frame"])
    return run_video_matte(model, wrap(tr, "frame", frames), skip=kw.pop("skip", 3), **kw)


def case_trimap_bgr(tr, m):
    return _single(tr, m, u8_frames(1, 7), trimap=trimap(2))


def case_trimap_rgb_events(tr, m):
    return _single(tr, m, with_events(u8_frames(3, 8), "f"), trimap=trimap(4), frames_are_rgb=True)


def case_alphas_u8_backgrounds_events(tr, m):
    return _single(tr, m, with_events(u8_frames(5, 7), "f"), alphas=alphas(6, 7), backgrounds=with_events(u8_frames(7, 7), "b"))


def case_alphas_float_rgb(tr, m):
    return _single(tr, m, float_frames(8, 7), alphas=alphas(9, 7), backgrounds=float_frames(10, 7), frames_are_rgb=True)


def case_u8_frames_float_backgrounds(tr, m):
    return _single(tr, m, with_events(u8_frames(11, 7), "f"), alphas=alphas(12, 7), backgrounds=float_frames(13, 7))


def case_keyframes_out_of_order(tr, m):
    return _single(tr, m, u8_frames(14, 8), keyframes={3: trimap(15), 5: trimap(16), 1: labels(17), 6: labels(18)},
                   gt_alpha_u8=plane_u8(19, 8), gt_mask="unknown")


def case_trimap_plus_keyframes(tr, m):
    return _single(tr, m, u8_frames(20, 8), trimap=trimap(21), keyframes={4: trimap(22), 2: labels(23)})


def case_large_input(tr, m):
    return _single(tr, m, u8_frames(24, 7, 1101, 1102), trimap=trimap(25, 1101, 1102), max_num=5)


def case_foreground_colour(tr, m):
    return _single(tr, m, u8_frames(26, 7), trimap=trimap(27), new_background=(10, 200, 30))


def case_foreground_one_image(tr, m):
    return _single(tr, m, u8_frames(28, 7), trimap=trimap(29), foreground=True, new_background=u8_frames(30, 1)[0])


def case_foreground_per_frame(tr, m):
    bgs = u8_frames(31, 7)
    return _single(tr, m, u8_frames(32, 7), trimap=trimap(33), new_background=[(1, 2, 3) if i == 2 else b for i, b in enumerate(bgs)])


def case_foreground_handed_over(tr, m):
    return _single(tr, m, u8_frames(34, 7), trimap=trimap(35), foreground=True, new_background=(0, 255, 7),
                   on_foreground=callbacks(tr)["on_foreground"], gt_alpha_u8=plane_u8(36, 7), gt_mask_u8=plane_u8(37, 7))


def _mask_clip(tr, m, h, w):
    from otvm_amd.masks import Mask
    return _single(tr, m, u8_frames(38, 8), mask=plane_u8(39, 1, h, w)[0],
                   keyframes={5: Mask(plane_u8(40, 1)[0].astype(np.float32) / 255, band=(2, 1.5), lo=100, hi=150, role="labels"),
                              3: Mask(plane_u8(41, 1)[0], band=2)})


def case_mask_and_mask_keyframes(tr, m):
    return _mask_clip(tr, m, H, W)


def case_mask_of_the_wrong_size(tr, m):
    return _mask_clip(tr, m, H, W + 1)


def case_masks_per_frame_working(tr, m):
    return _single(tr, m, with_events(u8_frames(42, 7), "f"), masks=plane_u8(43, 7), work_scale=2, frames_are_rgb=True)


def _working(tr, m, colour):
    return _single(tr, m, u8_frames(44, 7, 7, 9), wrap=ListSeq, trimap=trimap(45, 7, 9), keyframes={4: labels(46, 7, 9)},
                   work_scale=2, work_radius=3, work_eps=1e-3, foreground=True, new_background=colour)


def case_working_foreground_colour(tr, m):
    return _working(tr, m, (9, 8, 255))


def case_working_colour_out_of_range(tr, m):
    return _working(tr, m, (9, 8, 256))


def _batch(tr, model, clips, **kw):
    from otvm_amd.video import run_video_matte_batch
    clips = [Seq(tr, "frame %d" % b, c) for b, c in enumerate(clips)]
    for name in ("backgrounds", "alphas"):
        if name in kw:
            kw[name] = [Seq(tr, "%s %d" % (name[:-1], b), c) for b, c in enumerate(kw[name])]
    return run_video_matte_batch(model, clips, skip=3,
                                 on_frame=lambda b, i, alpha, u8, out: tr.ev("on_frame", b, i, alpha, u8, out[1]), **kw)


LENS = (5, 3, 1)


def case_batch_trimaps_events(tr, m):
    return _batch(tr, m, [with_events(u8_frames(50 + b, n), "c%df" % b) for b, n in enumerate(LENS)],
                  trimaps=[trimap(53 + b) for b in range(3)], frames_are_rgb=True)


def case_batch_alphas_float_backgrounds(tr, m):
    return _batch(tr, m, [u8_frames(56 + b, n) for b, n in enumerate(LENS)], alphas=[alphas(59 + b, n) for b, n in enumerate(LENS)],
                  backgrounds=[float_frames(62 + b, n) for b, n in enumerate(LENS)], frames_are_rgb=True)


def case_batch_foreground(tr, m):
    return _batch(tr, m, [u8_frames(65 + b, n) for b, n in enumerate(LENS)], trimaps=[trimap(68 + b) for b in range(3)],
                  new_background=[(5, 6, 7), u8_frames(71, 3), u8_frames(72, 1)[0]], gt_alpha_u8=[plane_u8(73 + b, n) for b, n in
                                                                                                 enumerate(LENS)], gt_mask="unknown")


def case_masks_per_frame_events(tr, m):
    """``masks`` at the frames' resolution, every frame with an upload event: the trimap is written per frame by the launch stream,
    so the event is waited for, not forwarded."""
    return _single(tr, m, with_events(u8_frames(80, 7), "f"), masks=plane_u8(81, 7), frames_are_rgb=True)


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}


def record(name, monkeypatch):
    """The trace of one case as plain data (what json.dumps takes)."""
    tr = Trace()
    install(monkeypatch, tr)
    model = StubModel(tr)
    try:
        res = CASES[name](tr, model)
        returned = [desc(r) | {"keys": sorted(r)} for r in (res if isinstance(res, list) else [res])]
    except ValueError as e:
        tr.ev("raised", type(e).__name__, str(e))
        returned = None
    return dict(events=tr.events, returned=returned, model_after=[model.foreground, desc(model._background)])
