"""Working-resolution matting, host side: the reductions and the guided upsampling of include/otvm_hip.h (otvm_downsample_*,
otvm_guided_coeffs, otvm_guided_apply) around device tensors.  Everything runs on the caller's current stream; there is no
PyTorch fallback."""
import ctypes as C

import torch

from . import lib as L

SCALES, RADII = (2, 3, 4), (1, 2, 3, 4)


def work_size(H, W, scale):
    return (H + scale - 1) // scale, (W + scale - 1) // scale


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _reduce(fn, name, src, dtype, lead, scale):
    if scale not in SCALES:
        raise ValueError("otvm_amd.guided: the scale is 2, 3 or 4, got %r" % (scale,))
    if src.dtype != dtype or not src.is_cuda:
        raise ValueError("otvm_amd.guided: %s takes a %s tensor on the GPU, got %s on %s" % (name, dtype, src.dtype, src.device))
    src = src.contiguous()
    H, W = (src.shape[-2:] if lead else src.shape[:2])
    h, w = work_size(H, W, scale)
    dst = torch.empty(((3, h, w) if lead else (h, w) + tuple(src.shape[2:])), dtype=dtype, device=src.device)
    L.check(fn(src.data_ptr(), H, W, scale, dst.data_ptr(), _stream(src.device)), name)
    return dst


def downsample_u8(frame, scale):
    """uint8 [H,W,3] -> [h,w,3]: rounded mean of each scale x scale block (clipped at the bottom / right edge)."""
    if frame.dim() != 3 or frame.shape[-1] != 3:
        raise ValueError("otvm_amd.guided: a frame is uint8 [H,W,3], got %s" % (tuple(frame.shape),))
    return _reduce(L.load().otvm_downsample_u8, "downsample_u8", frame, torch.uint8, False, scale)


def downsample_trimap(tri, scale):
    """one-hot float [3,H,W] -> [3,h,w]: fg / bg only where the whole block is; the unknown band never shrinks."""
    if tri.dim() != 3 or tri.shape[0] != 3:
        raise ValueError("otvm_amd.guided: a trimap is one-hot float [3,H,W], got %s" % (tuple(tri.shape),))
    return _reduce(L.load().otvm_downsample_trimap, "downsample_trimap", tri, torch.float32, True, scale)


def downsample_labels(labels, scale):
    """uint8 label map [H,W] -> [h,w]: 255 if a pixel of the block is unlabelled, the common class, otherwise 1 (unknown)."""
    if labels.dim() != 2:
        raise ValueError("otvm_amd.guided: a label map is uint8 [H,W], got %s" % (tuple(labels.shape),))
    return _reduce(L.load().otvm_downsample_labels, "downsample_labels", labels, torch.uint8, False, scale)


def foreground_bytes(alpha, fgr, rgb, background=None, who="otvm_amd.guided"):
    """RGBA [H,W,4] and, over ``background`` (a colour triple or a uint8 [H,W,3] device tensor), the composite [H,W,3] of an
    alpha plane [H,W] and the F planes [3,H,W] (fp32, unpadded): otvm_fgr_outputs.  Shared by the guided upsampler and the
    temporal stabilisation, which both remake the bytes from an alpha the engine did not write."""
    H, W = alpha.shape[-2:]
    device = alpha.device
    q = L.FgrParams()
    q.alpha_p, q.fgr_p = alpha.data_ptr(), fgr.data_ptr()
    q.Hp, q.Wp, q.H, q.W, q.lh, q.lw, q.u8_rgb = H, W, H, W, 0, 0, int(bool(rgb))
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device=device)
    q.rgba_u8 = rgba.data_ptr()
    comp = None
    if background is not None:
        comp = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        q.comp_u8 = comp.data_ptr()
        if torch.is_tensor(background):
            if background.dtype != torch.uint8 or tuple(background.shape) != (H, W, 3) or not background.is_contiguous():
                raise ValueError("%s: a background image is a contiguous uint8 [%d,%d,3] tensor (got %s %s)"
                                 % (who, H, W, background.dtype, tuple(background.shape)))
            q.bg_u8 = background.data_ptr()
        else:
            q.bg_color[:] = [int(c) for c in background]
    L.check(L.load().otvm_fgr_outputs(C.byref(q), _stream(device)), "fgr_outputs")
    return rgba, comp


class GuidedUpsampler:
    """Brings working-resolution targets (alpha, or alpha + the three F planes) back to H x W with the colour-guide fast guided
    filter.  Owns the coefficient buffers of one resolution (allocated once); the outputs are fresh tensors per call."""

    def __init__(self, device, H, W, scale, radius=2, eps=1e-4, channels=1):
        if scale not in SCALES:
            raise ValueError("GuidedUpsampler: the scale is 2, 3 or 4, got %r" % (scale,))
        if radius not in RADII:
            raise ValueError("GuidedUpsampler: the radius is 1 ... 4, got %r" % (radius,))
        if channels not in (1, 4):
            raise ValueError("GuidedUpsampler: 1 channel (alpha) or 4 (alpha + F), got %r" % (channels,))
        if not eps > 0:
            raise ValueError("GuidedUpsampler: eps must be positive, got %r" % (eps,))
        self.lib = L.load()
        self.device, self.H, self.W, self.scale, self.radius, self.eps, self.channels = device, H, W, scale, radius, float(eps), channels
        self.h, self.w = work_size(H, W, scale)
        self.ws = torch.empty(self.lib.otvm_guided_ws_bytes(self.h, self.w, channels), dtype=torch.uint8, device=device)
        self.coef = torch.empty((self.h, self.w, channels, 4), dtype=torch.float32, device=device)

    @property
    def coef_raw(self):
        """the un-averaged coefficients [h,w,C,4] of the last call (a view of the workspace)"""
        return self.ws.view(torch.float32).view(self.h, self.w, self.channels, 4)

    def reduce(self, frame):
        if tuple(frame.shape) != (self.H, self.W, 3):
            raise ValueError("GuidedUpsampler: frames are uint8 [%d,%d,3], got %s" % (self.H, self.W, tuple(frame.shape)))
        return downsample_u8(frame, self.scale)

    def _params(self):
        p = L.GuidedParams()
        p.H, p.W, p.s, p.h, p.w, p.r, p.C, p.eps = self.H, self.W, self.scale, self.h, self.w, self.radius, self.channels, self.eps
        p.coef = self.coef.data_ptr()
        return p

    def coeffs(self, work_frame, targets):
        """work_frame: uint8 [h,w,3]; targets: ``channels`` fp32 planes [h,w] (a list, or one [C,h,w] tensor)."""
        planes = [t.contiguous() for t in targets]
        if len(planes) != self.channels or any(tuple(t.shape) != (self.h, self.w) or t.dtype != torch.float32 for t in planes):
            raise ValueError("GuidedUpsampler: %d fp32 target planes [%d,%d] are needed" % (self.channels, self.h, self.w))
        work_frame = work_frame.contiguous()
        if tuple(work_frame.shape) != (self.h, self.w, 3) or work_frame.dtype != torch.uint8:
            raise ValueError("GuidedUpsampler: the working frame is uint8 [%d,%d,3]" % (self.h, self.w))
        p = self._params()
        p.guide_work = work_frame.data_ptr()
        for c, t in enumerate(planes):
            p.target[c] = t.data_ptr()
        L.check(self.lib.otvm_guided_coeffs(C.byref(p), self.ws.data_ptr(), _stream(self.device)), "guided_coeffs")

    def apply(self, frame):
        """frame: uint8 [H,W,3] -> (alpha [H,W] fp32, alpha_u8 [H,W], fgr [3,H,W] fp32 or None) from the stored coefficients."""
        frame = frame.contiguous()
        if tuple(frame.shape) != (self.H, self.W, 3) or frame.dtype != torch.uint8:
            raise ValueError("GuidedUpsampler: frames are uint8 [%d,%d,3]" % (self.H, self.W))
        alpha = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        u8 = torch.empty((self.H, self.W), dtype=torch.uint8, device=self.device)
        fgr = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.device) if self.channels == 4 else None
        p = self._params()
        p.guide_full, p.alpha, p.alpha_u8 = frame.data_ptr(), alpha.data_ptr(), u8.data_ptr()
        if fgr is not None:
            p.fgr = fgr.data_ptr()
        L.check(self.lib.otvm_guided_apply(C.byref(p), _stream(self.device)), "guided_apply")
        return alpha, u8, fgr

    def upsample(self, frame, work_frame, targets):
        self.coeffs(work_frame, targets)
        return self.apply(frame)

    def foreground_bytes(self, alpha, fgr, rgb, background=None):
        """RGBA [H,W,4] and, over ``background`` (a colour triple or a uint8 [H,W,3] device tensor), the composite [H,W,3]:
        otvm_fgr_outputs on the full-resolution planes (no padding)."""
        return foreground_bytes(alpha, fgr, rgb, background, "GuidedUpsampler")
