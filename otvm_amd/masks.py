"""Trimaps from segmentation masks, host side: otvm_trimap_from_mask (include/otvm_hip.h) around device tensors, and the ``Mask``
value object run_video_matte takes wherever it takes a trimap or a label map.  Everything runs on the caller's current stream;
there is no PyTorch fallback.

The default thresholds (lo = 127, hi = 128: a binary cut of an 8-bit mask) and the default band (the model's DILATION_KERNEL) are
PLACEHOLDERS: nobody has tuned them on real footage."""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L

ROLES = ("key", "labels")


def band_thresholds(band):
    """``band`` -- r, or (r_fg, r_bg), real radii in pixels, 0 ... 255 -- as the integer thresholds (t_fg, t_bg), t = floor(r^2)."""
    pair = tuple(band) if isinstance(band, (tuple, list)) else (band, band)
    if len(pair) != 2:
        raise ValueError("otvm_amd.masks: band is a radius r or a pair (r_fg, r_bg), got %r" % (band,))
    out = []
    for r in pair:
        if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not 0 <= r <= 255:
            raise ValueError("otvm_amd.masks: a band radius is a number in 0 ... 255 pixels, got %r" % (r,))
        out.append(int(math.floor(float(r) * float(r))))
    return out[0], out[1]


def check_thresholds(lo, hi):
    if isinstance(lo, bool) or isinstance(hi, bool) or not isinstance(lo, (int, np.integer)) or not isinstance(hi, (int, np.integer)):
        raise ValueError("otvm_amd.masks: the thresholds lo, hi are integers, got %r, %r" % (lo, hi))
    if not 0 <= lo < hi <= 255:
        raise ValueError("otvm_amd.masks: the thresholds need 0 <= lo < hi <= 255 (lo >= hi leaves no class apart), got lo=%r hi=%r"
                         % (lo, hi))
    return int(lo), int(hi)


def quantise(mask):
    """A float mask in [0,1] -> uint8, once: (m.clamp(0, 1) * 255 + 0.5).to(torch.uint8); a uint8 mask is used as it is."""
    if mask.dtype == torch.uint8:
        return mask
    if not mask.dtype.is_floating_point:
        raise ValueError("otvm_amd.masks: a mask is uint8 (0 ... 255) or float in [0,1], got %s" % mask.dtype)
    return (mask.float().clamp(0, 1) * 255 + 0.5).to(torch.uint8)


class MaskTrimapper:
    """otvm_trimap_from_mask for one resolution: owns the workspace (allocated once, no initialisation needed); the outputs are
    fresh tensors per call.  One instance serves one stream at a time."""

    def __init__(self, device, H, W):
        self.lib = L.load()
        n = self.lib.otvm_trimap_from_mask_ws_bytes(int(H), int(W))
        if n < 0:
            raise ValueError("otvm_amd.masks: a mask is 1 ... 16383 pixels a side, got %dx%d" % (H, W))
        self.device, self.H, self.W = device, int(H), int(W)
        self.ws = torch.empty(n, dtype=torch.uint8, device=device)

    def __call__(self, mask, t_fg, t_bg, lo, hi, labels=False, band_label=1):
        """mask: uint8 [H,W] on the device -> one-hot float [3,H,W] (bg, unknown, fg), or with ``labels`` the uint8 [H,W] label
        map (0 bg, 2 fg, ``band_label`` in the band)."""
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (self.H, self.W) or mask.device != self.ws.device:
            raise ValueError("otvm_amd.masks: the mask is uint8 [%d,%d] on %s, got %s %s on %s"
                             % (self.H, self.W, self.ws.device, mask.dtype, tuple(mask.shape), mask.device))
        mask = mask.contiguous()
        p = L.MaskTrimapParams()
        p.mask, p.H, p.W, p.lo, p.hi, p.t_fg, p.t_bg, p.band_label = mask.data_ptr(), self.H, self.W, lo, hi, t_fg, t_bg, band_label
        if labels:
            out = torch.empty((self.H, self.W), dtype=torch.uint8, device=self.ws.device)
            p.labels = out.data_ptr()
        else:
            out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.ws.device)
            p.trimap = out.data_ptr()
        L.check(self.lib.otvm_trimap_from_mask(C.byref(p), self.ws.data_ptr(), torch.cuda.current_stream(self.ws.device).cuda_stream),
                "trimap_from_mask")
        return out


_TRIMAPPERS = {}       # (device, H, W, stream) -> MaskTrimapper: one workspace per resolution and stream


def trimap_from_mask(mask, band, lo=127, hi=128, labels=False, band_label=1):
    """Device mask [H,W] (uint8, or float in [0,1], quantised once) -> one-hot trimap float [3,H,W], or with ``labels`` the uint8
    label map [H,W] with ``band_label`` (1 unknown, 255 unlabelled) in the band.  ``band``: r or (r_fg, r_bg) in pixels -- how far
    the unknown band reaches into the foreground / the background of the thresholded mask (Euclidean, exact).  On the current
    stream."""
    if not torch.is_tensor(mask) or not mask.is_cuda or mask.dim() != 2:
        raise ValueError("otvm_amd.masks: trimap_from_mask takes a [H,W] tensor on the GPU")
    t_fg, t_bg = band_thresholds(band)
    lo, hi = check_thresholds(lo, hi)
    if band_label not in (1, 255):
        raise ValueError("otvm_amd.masks: band_label is 1 (unknown) or 255 (unlabelled), got %r" % (band_label,))
    H, W = mask.shape
    key = (mask.device, int(H), int(W), torch.cuda.current_stream(mask.device).cuda_stream)
    tm = _TRIMAPPERS.get(key)
    if tm is None:
        if len(_TRIMAPPERS) >= 8:
            _TRIMAPPERS.clear()                    # (a handful of resolutions per process; nothing grows without bound)
        tm = _TRIMAPPERS[key] = MaskTrimapper(mask.device, H, W)
    return tm(quantise(mask), t_fg, t_bg, lo, hi, labels=bool(labels), band_label=int(band_label))


class Mask:
    """A segmentation mask where run_video_matte takes a trimap or a label map: ``data`` [H,W], uint8 (0 ... 255) or float in
    [0,1], binary or soft; ``band`` = r or (r_fg, r_bg) in pixels (None: the model's DILATION_KERNEL); FG = data >= hi, BG =
    data <= lo on the 8-bit scale.  role="key": the trimap of a full keyframe.  role="labels": a correction -- 0 / 2 in the sure
    regions, 255 (unlabelled) in the band, so the propagated trimap survives there."""

    def __init__(self, data, band=None, lo=127, hi=128, role="key"):
        if role not in ROLES:
            raise ValueError("Mask: role is 'key' (a full keyframe) or 'labels' (a correction), got %r" % (role,))
        nd = data.dim() if torch.is_tensor(data) else np.asarray(data).ndim
        if nd != 2:
            raise ValueError("Mask: a mask is one plane [H,W], got %d dimensions" % nd)
        dt = data.dtype if torch.is_tensor(data) else np.asarray(data).dtype
        ok = (dt == torch.uint8 or dt.is_floating_point) if torch.is_tensor(data) else (dt == np.uint8 or dt.kind == "f")
        if not ok:
            raise ValueError("Mask: a mask is uint8 (0 ... 255) or float in [0,1], got %s" % dt)
        if band is not None:
            band_thresholds(band)
        self.lo, self.hi = check_thresholds(lo, hi)
        self.data, self.band, self.role = data, band, role

    @property
    def shape(self):
        return tuple(self.data.shape)

    def band_for(self, model):
        """This mask's band, or the model's DILATION_KERNEL when it names none."""
        if self.band is not None:
            return self.band
        core = model.module if hasattr(model, "module") else model
        dk = getattr(core, "DILATION_KERNEL", None)
        if dk is None:
            raise ValueError("Mask: no band given and the model has no DILATION_KERNEL to take one from; pass band=r (pixels)")
        band_thresholds(dk)
        return dk

    def convert(self, model, device):
        """-> the one-hot trimap [3,H,W] (role "key") or the label map [H,W] (role "labels") on ``device``."""
        t = self.data
        if not torch.is_tensor(t):
            a = np.ascontiguousarray(t)
            t = torch.from_numpy(a if a.flags.writeable else a.copy())     # (PIL hands out read-only buffers)
        return trimap_from_mask(t.to(device), self.band_for(model), self.lo, self.hi, labels=self.role == "labels", band_label=255)


def as_mask(x, what):
    """An array / tensor [H,W] stands for Mask(x) with the defaults."""
    if isinstance(x, Mask):
        return x
    try:
        return Mask(x)
    except ValueError as e:
        raise ValueError("%s: %s" % (what, e)) from None
