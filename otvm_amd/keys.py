"""Masks of keyed footage, host side: otvm_mask_from_chroma and otvm_mask_from_plate (include/otvm_hip.h) around device tensors,
and the two key objects run_video_matte takes as ``key=``.  Footage shot against a green or blue screen, and locked-off shots with
a clean plate of the empty set, need no hand-made mask: the mask of every frame is made on the device from the frame itself --
255 subject, 0 screen / plate, what otvm_trimap_from_mask expects -- and the ``masks=`` route does the rest.  Everything runs on the
caller's current stream; there is no PyTorch fallback.

  * ``ChromaKey``: a hue-cone key that does not depend on brightness.  Cb, Cr of a pixel (BT.601 full range, the integers of
    otvm_rgb_to_yuv420's chroma rows), q = dot - |cross| against the key colour's (kb, kr): positive inside the 45 degree cone round
    the key's hue, growing with saturation; a ramp between the thresholds.
  * ``PlateKey``: a difference key.  d = min over the (2r+1)^2 neighbourhood of the PLATE of max_c |I_c - P_c|; a ramp between the
    thresholds.  The neighbourhood minimum absorbs sub-pixel camera jitter and sensor noise.
  * ``key_mask(frame, key)`` is the launch alone.

Every default below -- the thresholds of both keys, the radius, the cut of the mask (mask_lo, mask_hi) and the band (the model's
DILATION_KERNEL) -- is a PLACEHOLDER: nobody has tuned them on real footage.  The kernels are CHECKED BY DEFINITION ONLY (bit for
bit against tests/key_ref.py); with no trained checkpoint here nothing is claimed about matting quality.  Out of scope: estimating
the key colour, despill (the network's F is the project's answer), despeckling the key, a moving-camera plate."""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from .masks import Mask, band_thresholds, check_thresholds, trimap_from_mask

COLOURS = {"green": (0, 255, 0), "blue": (0, 0, 255)}
CH, UR, VB = 524288, 176932, 85262        # the chroma rows of BT.601 full range, 20 fractional bits (otvm_rgb_to_yuv420's)


def chroma_of(rgb):
    """(cb, cr) = (Cb - 128, Cr - 128) of one (R, G, B), by the kernel's rule: 20 fractional bits, one round-half-up, one clamp."""
    r, g, b = (int(v) for v in rgb)
    bias = (128 << 20) + (1 << 19)
    cb = min(255, max(0, (-UR * r - (CH - UR) * g + CH * b + bias) >> 20)) - 128
    cr = min(255, max(0, (CH * r - (CH - VB) * g - VB * b + bias) >> 20)) - 128
    return cb, cr


def _round(x):
    return int(math.floor(x + 0.5))


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


class _Key:
    """What both keys carry for the mask-to-trimap step: the band (None: the model's DILATION_KERNEL) and the cut of the mask."""

    def __init__(self, band, mask_lo, mask_hi):
        if band is not None:
            band_thresholds(band)
        self.band = band
        self.mask_lo, self.mask_hi = check_thresholds(mask_lo, mask_hi)


class ChromaKey(_Key):
    """``colour``: "green" (0,255,0), "blue" (0,0,255) or an (R, G, B) triple picked from the footage.  ``lo`` < ``hi``: thresholds
    of q / |K| in chroma code values -- the mask is 255 (subject) up to lo, 0 (screen) from hi, a ramp between.  They become the
    kernel's integers once, here: qlo = round(lo |K|), qhi = round(hi |K|), |K| = sqrt(kb^2 + kr^2) in float64 -- the only
    floating-point step.  A grey key colour (kb^2 + kr^2 < 16^2) is refused.  ``band``, ``mask_lo``, ``mask_hi``: masks.Mask's.
    The defaults (8, 24; 127, 128; the model's band) are PLACEHOLDERS nobody has tuned on real footage."""

    def __init__(self, colour, lo=8, hi=24, band=None, mask_lo=127, mask_hi=128):
        if isinstance(colour, str):
            if colour not in COLOURS:
                raise ValueError("ChromaKey: colour is 'green', 'blue' or an (R, G, B) triple, got %r" % (colour,))
            colour = COLOURS[colour]
        try:
            ok = len(colour) == 3 and all(not isinstance(v, bool) and int(v) == v and 0 <= int(v) <= 255 for v in colour)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("ChromaKey: colour is 'green', 'blue' or an (R, G, B) triple of integers 0 ... 255, got %r" % (colour,))
        self.colour = tuple(int(v) for v in colour)
        self.kb, self.kr = chroma_of(self.colour)
        k2 = self.kb * self.kb + self.kr * self.kr
        if k2 < 256:
            raise ValueError("ChromaKey: the key colour %r is grey (its chroma is (%d, %d), shorter than 16): it has no hue to key on"
                             % (self.colour, self.kb, self.kr))
        if not (_number(lo) and _number(hi)) or not lo < hi or abs(lo) > 256 or abs(hi) > 256:
            raise ValueError("ChromaKey: the thresholds need lo < hi (chroma code values, within +-256), got lo=%r hi=%r" % (lo, hi))
        self.lo, self.hi = lo, hi
        norm = math.sqrt(float(k2))
        self.qlo, self.qhi = _round(float(lo) * norm), _round(float(hi) * norm)
        if not self.qlo < self.qhi:
            raise ValueError("ChromaKey: the thresholds lo=%r hi=%r leave no ramp (qlo = qhi = %d)" % (lo, hi, self.qlo))
        super().__init__(band, mask_lo, mask_hi)

    def check_frames(self, H, W):
        pass


class PlateKey(_Key):
    """``plate``: the clean plate, uint8 [H,W,3], an array or a tensor, in the frames' channel order; uploaded once per clip.
    Integers 0 <= ``lo`` < ``hi`` <= 255: the mask is 0 (plate) up to lo, 255 (subject) from hi, a ramp between; ``radius`` 0 ... 3:
    the neighbourhood of the plate the minimum is taken over.  ``band``, ``mask_lo``, ``mask_hi``: masks.Mask's.  The defaults
    (12, 40; 1; 127, 128; the model's band) are PLACEHOLDERS nobody has tuned on real footage."""

    def __init__(self, plate, lo=12, hi=40, radius=1, band=None, mask_lo=127, mask_hi=128):
        shape = tuple(plate.shape) if hasattr(plate, "shape") else ()
        dt = getattr(plate, "dtype", None)
        if len(shape) != 3 or shape[2] != 3 or dt not in (torch.uint8, np.uint8, np.dtype("uint8")):
            raise ValueError("PlateKey: the plate is uint8 [H,W,3], got %s %s" % (dt, shape))
        try:
            self.lo, self.hi = check_thresholds(lo, hi)
        except ValueError:
            raise ValueError("PlateKey: the thresholds are integers with 0 <= lo < hi <= 255, got lo=%r hi=%r" % (lo, hi)) from None
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= 3:
            raise ValueError("PlateKey: radius is 0 ... 3, got %r" % (radius,))
        self.plate, self.radius = plate, int(radius)
        self._on = None
        super().__init__(band, mask_lo, mask_hi)

    @property
    def shape(self):
        return tuple(self.plate.shape[:2])

    def check_frames(self, H, W):
        if self.shape != (H, W):
            raise ValueError("run_video_matte: the plate of `key` is %dx%d, the frames are %dx%d (a plate is given at the frames' "
                             "resolution)" % (self.shape + (H, W)))

    def on(self, device):
        """The plate on ``device``, uploaded once."""
        if self._on is None or self._on.device != torch.device(device):
            t = self.plate
            if not torch.is_tensor(t):
                a = np.ascontiguousarray(t)
                t = torch.from_numpy(a if a.flags.writeable else a.copy())
            self._on = t.to(device).contiguous()
        return self._on


def check_key(key, who="run_video_matte"):
    if not isinstance(key, (ChromaKey, PlateKey)):
        raise ValueError("%s: `key` is a keys.ChromaKey or a keys.PlateKey, got %r" % (who, type(key).__name__))
    return key


def key_mask(frame, key, rgb=False, out=None):
    """The launch alone: ``frame`` uint8 [H,W,3] on the device (R, G, B when ``rgb``, else B, G, R) -> the key's mask uint8 [H,W],
    255 subject, 0 screen / plate, on the current stream.  To key only the first frame and propagate:
    run_video_matte(..., mask=Mask(keys.key_mask(f0, key).cpu()))."""
    check_key(key, "otvm_amd.keys.key_mask")
    if not (torch.is_tensor(frame) and frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3):
        raise ValueError("otvm_amd.keys: key_mask takes a uint8 [H,W,3] tensor on the GPU (float frames have no key route)")
    frame = frame.contiguous()
    H, W = frame.shape[:2]
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=frame.device)
    stream = torch.cuda.current_stream(frame.device).cuda_stream
    if isinstance(key, ChromaKey):
        p = L.MaskFromChromaParams(frame=frame.data_ptr(), mask=out.data_ptr(), H=H, W=W, u8_rgb=int(bool(rgb)), kb=key.kb, kr=key.kr,
                                   qlo=key.qlo, qhi=key.qhi)
        L.check(L.load().otvm_mask_from_chroma(C.byref(p), stream), "mask_from_chroma")
    else:
        if key.shape != (H, W):
            raise ValueError("otvm_amd.keys: the plate is %dx%d, the frame %dx%d" % (key.shape + (H, W)))
        plate = key.on(frame.device)
        p = L.MaskFromPlateParams(frame=frame.data_ptr(), plate=plate.data_ptr(), mask=out.data_ptr(), H=H, W=W, radius=key.radius,
                                  lo=key.lo, hi=key.hi)
        L.check(L.load().otvm_mask_from_plate(C.byref(p), stream), "mask_from_plate")
    return out


class KeyedMask(Mask):
    """A key bound to a frame, where run_video_matte takes the Mask of that frame: ``bind`` hands over the frame AS IT IS STAGED ON
    THE DEVICE (no second upload), ``convert`` runs the key launch on it and then masks.trimap_from_mask -- so the per-frame
    machinery of ``masks=`` sees an ordinary per-frame source.  ``shape`` is None: the mask has the frame's size by construction."""

    def __init__(self, key, rgb):
        self.key, self.rgb = check_key(key), bool(rgb)
        self.data, self.frame = None, None
        self.band, self.lo, self.hi, self.role = key.band, key.mask_lo, key.mask_hi, "key"

    @property
    def shape(self):
        return None

    def bind(self, frame):
        self.frame = frame

    def convert(self, model, device):
        if self.frame is None:
            raise RuntimeError("otvm_amd.keys: a key is converted on the frame staged for it; none is bound")
        return trimap_from_mask(key_mask(self.frame, self.key, self.rgb), self.band_for(model), self.lo, self.hi)
