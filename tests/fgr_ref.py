"""numpy restatement of otvm_fgr_outputs (include/otvm_hip.h): every step one float32 IEEE operation, in the kernel's order."""
import numpy as np

F32 = np.float32


def quant_u8(v, ok=True):
    """(uint8) trunc(v * 255), clamped to the byte range; a non-finite operand (or ``ok`` False) gives 0."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.minimum(np.maximum(np.trunc(v * F32(255.0)), F32(0.0)), F32(255.0))
    fin = np.isfinite(v) & ok
    return np.where(fin, t, F32(0.0)).astype(np.uint8)


def fgr_outputs(alpha, F, bg=None, u8_rgb=False):
    """alpha [H,W], F [3,H,W] (R, G, B) float32; bg: None, uint8 [H,W,3] or a colour triple, in the outputs' channel order.
    Returns (fgr [3,H,W], rgba_u8 [H,W,4], comp_u8 [H,W,3] or None)."""
    alpha, F = np.asarray(alpha, F32), np.asarray(F, F32)
    order = (0, 1, 2) if u8_rgb else (2, 1, 0)
    rgba = np.stack([quant_u8(F[c]) for c in order] + [quant_u8(alpha)], -1)
    comp = None
    if bg is not None:
        bg = np.broadcast_to(np.asarray(bg, np.uint8), alpha.shape + (3,))
        ch = []
        with np.errstate(invalid="ignore", over="ignore"):
            for j, c in enumerate(order):
                bgf = bg[..., j].astype(F32) * (F32(1.0) / F32(255.0))
                v = (F[c] * alpha) + (bgf * (F32(1.0) - alpha))
                ch.append(quant_u8(v, np.isfinite(F[c]) & np.isfinite(alpha)))
        comp = np.stack(ch, -1)
    return F.copy(), rgba, comp
