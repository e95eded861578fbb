"""otvm_subjects_resolve restated in numpy, operation by operation in fp32 (the kernel is compiled with -ffp-contract=off and
compared bit for bit).  The integer track policy is not restated here: it is otvm_amd.roi.track_origin."""
import numpy as np

from tests.roi_ref import quant_u8
from tests.roi_track_ref import clamp_origin as _clamp_origin

F32 = np.float32


def clamp_origin(origin, size, H, W):
    """What the kernels make of an origin row: roi_track_ref's clamp to [0, H - h] x [0, W - w], the size as one argument."""
    return _clamp_origin(origin, size[0], size[1], H, W)


def resolve(origins, size, H, W, alphas, trimaps, fgrs=None, frame=None, u8_rgb=False, normalise=False):
    """origins: S x (y0, x0) as logged (clamped here as the kernel clamps them); alphas S x [h,w]; trimaps S x [3,h,w]; fgrs
    S x [3,h,w] or None.  -> dict(alpha [S,H,W], alpha_u8, trimap [S,3,H,W], fgr [S,3,H,W] or None, union [H,W], union_u8, owner)."""
    S, (h, w) = len(alphas), size
    a = np.zeros((S, H, W), F32)                                  # 1. outside its window a subject is background: 0.f
    tri = np.zeros((S, 3, H, W), F32)
    tri[:, 0] = F32(1.0)                                          # 6. (1, 0, 0) outside
    F = None
    if fgrs is not None:
        order = (0, 1, 2) if u8_rgb else (2, 1, 0)
        s255 = F32(1.0) / F32(255.0)
        outside = np.stack([np.asarray(frame)[..., order[c]].astype(F32) * s255 for c in range(3)]).astype(F32)
        F = np.repeat(outside[None], S, axis=0)                   # 7. the frame's pixel outside
    for s in range(S):
        y0, x0 = clamp_origin(origins[s], size, H, W)
        a[s, y0:y0 + h, x0:x0 + w] = np.asarray(alphas[s], F32)
        tri[s, :, y0:y0 + h, x0:x0 + w] = np.asarray(trimaps[s], F32)
        if F is not None:
            F[s, :, y0:y0 + h, x0:x0 + w] = np.asarray(fgrs[s], F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        total = a[0].copy()                                       # 2. ((a_0 + a_1) + a_2) + ...
        for s in range(1, S):
            total = (total + a[s]).astype(F32)
        union = np.fmin(total, F32(1.0)).astype(F32)              # 8. fminf of the UNNORMALISED sum (a NaN sum gives 1.f)
        if normalise:                                             # 3. a NaN sum fails the comparison: nothing is rescaled
            over = total > F32(1.0)
            for s in range(S):
                a[s] = np.where(over, (a[s] / np.where(over, total, F32(1.0))).astype(F32), a[s])
        best = np.zeros((H, W), F32)                              # 9. the smallest s whose a_s is largest and > 0.f
        owner = np.full((H, W), 255, np.uint8)
        for s in range(S):
            better = a[s] > best
            best = np.where(better, a[s], best)
            owner = np.where(better, np.uint8(s), owner).astype(np.uint8)
    return dict(alpha=a, alpha_u8=np.stack([quant_u8(a[s]) for s in range(S)]), trimap=tri, fgr=F, union=union,
                union_u8=quant_u8(union), owner=owner)
