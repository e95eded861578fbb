"""Temporal stabilisation of alpha, host side: a causal, one-frame-state, flow-compensated recursive filter around the device
kernels of include/otvm_hip.h (otvm_luma_u8, otvm_optflow_farneback, otvm_temporal_blend).  Everything runs on the caller's
current stream; there is no PyTorch fallback.

There is no trained checkpoint here: the filter is checked by definition and by property on synthetic clips, not by quality on
real footage.  The default parameters (strength, tau_colour, tau_alpha) are PLACEHOLDERS: nobody has tuned them on real footage."""
import ctypes as C

import numpy as np
import torch

from . import lib as L

REGIONS = ("unknown", "all")


def check_options(strength=0.5, tau_colour=24.0, tau_alpha=0.5, region="unknown"):
    """The constructor's refusals (host only): (strength, inv_tau_colour, inv_tau_alpha) as the kernel takes them -- the
    reciprocals in float32 -- and the region."""
    try:
        k, tc, ta = float(strength), float(tau_colour), float(tau_alpha)
    except (TypeError, ValueError):
        raise ValueError("TemporalStabiliser: strength, tau_colour and tau_alpha are numbers, got %r, %r, %r"
                         % (strength, tau_colour, tau_alpha))
    if isinstance(strength, bool) or not 0.0 <= k <= 1.0:
        raise ValueError("TemporalStabiliser: strength lies in [0,1], got %r" % (strength,))
    if not (tc > 0 and np.isfinite(tc)) or not (ta > 0 and np.isfinite(ta)):
        raise ValueError("TemporalStabiliser: tau_colour (grey levels) and tau_alpha are positive, got %r and %r" % (tau_colour, tau_alpha))
    with np.errstate(divide="ignore", over="ignore"):
        itc, ita = np.float32(1.0) / np.float32(tc), np.float32(1.0) / np.float32(ta)
    if not (np.isfinite(itc) and itc > 0 and np.isfinite(ita) and ita > 0):
        raise ValueError("TemporalStabiliser: 1 / tau_colour and 1 / tau_alpha must be float32 numbers, got taus %r and %r"
                         % (tau_colour, tau_alpha))
    if region not in REGIONS:
        raise ValueError("TemporalStabiliser: region is 'unknown' (only the trimap's unknown class is filtered) or 'all', got %r"
                         % (region,))
    return float(np.float32(k)), float(itc), float(ita), region


def options_of(stabilise):
    """run_video_matte's ``stabilise`` -> the constructor's keywords (checked), or None when the option is off."""
    if stabilise is None or stabilise is False:
        return None
    if stabilise is True:
        kw = {}
    elif isinstance(stabilise, dict):
        kw = dict(stabilise)
        unknown = sorted(set(kw) - {"strength", "tau_colour", "tau_alpha", "region"})
        if unknown:
            raise ValueError("stabilise: a dict holds TemporalStabiliser's keywords strength, tau_colour, tau_alpha, region; got %s"
                             % ", ".join(unknown))
    elif isinstance(stabilise, (int, float)):
        kw = {"strength": float(stabilise)}
    else:
        raise ValueError("stabilise is None, True, a strength in [0,1] or a dict of TemporalStabiliser's keywords, got %r"
                         % (stabilise,))
    check_options(**kw)
    return kw


class TemporalStabiliser:
    """alpha_t <- alpha_t + w * (warp(stabilised alpha_{t-1}) - alpha_t), w = strength * wc * wa * gate per pixel
    (include/otvm_hip.h, otvm_temporal_blend): the previous output is fetched where the Farneback flow of the grey frames
    points, wc falls to 0 as the grey residual there reaches ``tau_colour`` (grey levels; an occlusion or a wrong flow), wa as
    the change of alpha reaches ``tau_alpha`` (a real change is not smoothed away), and with region="unknown" only pixels whose
    trimap class is unknown are touched.  strength = 0 is the identity (the clamped alpha).

    Owns the flow workspace, the flow plane and two grey planes of one resolution (allocated once); the state is the previous
    output tensor -- the tensors step() returns are fresh, and the caller must not write into the alpha it was handed before
    the next step.  The defaults are PLACEHOLDERS: nobody has tuned them on real footage."""

    def __init__(self, device, H, W, strength=0.5, tau_colour=24.0, tau_alpha=0.5, region="unknown"):
        self.strength, self.inv_tau_colour, self.inv_tau_alpha, self.region = check_options(strength, tau_colour, tau_alpha, region)
        if not (1 <= int(H) <= 65535 and int(W) >= 1):
            raise ValueError("TemporalStabiliser: H is 1 ... 65535 and W >= 1, got %r x %r" % (W, H))
        self.lib = L.load()
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device, self.H, self.W = device, int(H), int(W)
        self.ws = torch.empty(self.lib.otvm_optflow_farneback_ws_bytes(self.H, self.W), dtype=torch.uint8, device=self.device)
        self.flow = torch.empty((self.H, self.W, 2), dtype=torch.float32, device=self.device)
        self.grey = [torch.empty((self.H, self.W), dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.reset()

    def reset(self):
        """Forget the previous frame: the next step starts a clip."""
        self.state, self.cur, self.last_flow = None, 0, None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, frame_u8, alpha, trimap, tri_scale):
        H, W = self.H, self.W
        for name, t, dtype, shape in (("the frame", frame_u8, torch.uint8, (H, W, 3)), ("alpha", alpha, torch.float32, (H, W))):
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != self.device:
                raise ValueError("TemporalStabiliser: %s is a %s tensor %s on %s, got %s"
                                 % (name, str(dtype).replace("torch.", ""), list(shape), self.device,
                                    "%s %s on %s" % (t.dtype, list(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
        if self.region == "all":
            return None
        if trimap is None:
            raise ValueError("TemporalStabiliser: region='unknown' filters the trimap's unknown class: step() needs the trimap "
                             "(region='all' takes none)")
        if isinstance(tri_scale, bool) or not isinstance(tri_scale, int) or tri_scale < 1:
            raise ValueError("TemporalStabiliser: tri_scale is a positive integer, got %r" % (tri_scale,))
        th, tw = (H + tri_scale - 1) // tri_scale, (W + tri_scale - 1) // tri_scale
        if (not torch.is_tensor(trimap) or trimap.dtype != torch.float32 or tuple(trimap.shape) != (3, th, tw)
                or trimap.device != self.device):
            raise ValueError("TemporalStabiliser: the trimap is a float32 tensor [3,%d,%d] on %s (tri_scale %d), got %s"
                             % (th, tw, self.device, tri_scale,
                                "%s %s on %s" % (trimap.dtype, list(trimap.shape), trimap.device) if torch.is_tensor(trimap)
                                else type(trimap).__name__))
        return trimap.contiguous()

    def step(self, frame_u8, alpha, trimap=None, tri_scale=1, rgb=False):
        """frame_u8: uint8 [H,W,3] (B,G,R unless ``rgb``); alpha: this frame's raw alpha, fp32 [H,W]; trimap: fp32 [3,th,tw]
        (bg, unknown, fg; th, tw = ceil(H / tri_scale), ceil(W / tri_scale)) -- needed with region="unknown", ignored with
        "all".  Returns (stabilised alpha fp32 [H,W] in [0,1], its byte trunc(alpha * 255) uint8 [H,W]), fresh tensors.  The
        first step after construction or reset() returns the clamped alpha."""
        tri = self._check(frame_u8, alpha, trimap, tri_scale)
        st = self._stream()
        frame_u8, alpha = frame_u8.contiguous(), alpha.contiguous()
        grey, grey_prev = self.grey[self.cur], self.grey[1 - self.cur]
        L.check(self.lib.otvm_luma_u8(frame_u8.data_ptr(), self.H, self.W, int(bool(rgb)), grey.data_ptr(), st), "luma_u8")
        out = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        u8 = torch.empty((self.H, self.W), dtype=torch.uint8, device=self.device)
        p = L.TemporalParams()
        p.H, p.W, p.alpha, p.out, p.out_u8 = self.H, self.W, alpha.data_ptr(), out.data_ptr(), u8.data_ptr()
        p.strength, p.inv_tau_colour, p.inv_tau_alpha = self.strength, self.inv_tau_colour, self.inv_tau_alpha
        if self.state is not None:
            # the flow from this frame to the previous one: where each pixel of this frame was
            L.check(self.lib.otvm_optflow_farneback(grey.data_ptr(), grey_prev.data_ptr(), self.H, self.W, self.flow.data_ptr(),
                                                    self.ws.data_ptr(), st), "optflow_farneback")
            self.last_flow = self.flow
            p.prev, p.grey, p.grey_prev, p.flow = self.state.data_ptr(), grey.data_ptr(), grey_prev.data_ptr(), self.flow.data_ptr()
            if tri is not None:
                p.tri, p.th, p.tw, p.tri_scale = tri.data_ptr(), tri.shape[1], tri.shape[2], tri_scale
        L.check(self.lib.otvm_temporal_blend(C.byref(p), st), "temporal_blend")
        self.state, self.cur = out, 1 - self.cur
        return out, u8
