"""CPU restatement of the Grad and Conn matting metrics (reference utils/tmp/metric.py:16-46,191-234).  TEST INFRASTRUCTURE.

Inputs are uint8 [H,W] pred / target and an optional uint8 {0,1} mask, as otvm_matting_grad_conn takes them.

Grad : (|grad p| - |grad t|)^2 * m summed, grad = the 9x9 Gaussian-derivative filter of sigma 1.4 as a true convolution with
       replicate padding.  Restated in float64 with the separable factors of hx (hx = g (x) dg / |g| |dg|).
Conn : the level map of BatchConnectivity (10 float32 thresholds, largest 4-connected component per threshold, first
       component in raster order among equal sizes), then |phi_p - phi_t| * m in float32 exactly as the reference computes
       it; the sum in float64.
The fixture tests/golden/metrics_grad_conn.npz (make_metric_golden.py) pins both against the reference's own functions.
"""
import math

import numpy as np
from scipy import ndimage

SIGMA, THETA = 1.4, 0.15
CROSS = ndimage.generate_binary_structure(2, 1)          # 4-connectivity (skimage connectivity=1)


def levels():
    """t_k = float32(0 + k * 0.1) for k = 0..10 -- torch.arange(0, 1.1, 0.1) on the CPU (start + k * step in double)."""
    return np.array([0.0 + k * 0.1 for k in range(11)], np.float64).astype(np.float32)


def cutoffs():
    """c_i (i = 1..10): x >= c_i  <=>  float32(x) / 255 >= t_i  for x in 0..255."""
    t = levels()
    x = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.array([int(np.argmax(x >= t[i])) if (x >= t[i]).any() else 256 for i in range(1, 11)])


def grad_taps():
    """(g[9], dg[9]) in float64: genGaussKernel's factors sampled at -4..4, each normalised to unit L2 norm."""
    hsize = int(math.ceil(SIGMA * math.sqrt(-2 * math.log(math.sqrt(2 * math.pi) * SIGMA * 1e-2))))
    x = np.arange(-hsize, hsize + 1, dtype=np.float64)
    g = np.exp(-x ** 2 / (2 * SIGMA ** 2)) / (SIGMA * math.sqrt(2 * math.pi))
    dg = -x * g / SIGMA ** 2
    return g / np.sqrt((g ** 2).sum()), dg / np.sqrt((dg ** 2).sum())


def grad_amplitude(u8):
    g, dg = grad_taps()
    x = np.asarray(u8, np.float64) / 255.0
    gx = ndimage.convolve1d(ndimage.convolve1d(x, dg, axis=1, mode="nearest"), g, axis=0, mode="nearest")
    gy = ndimage.convolve1d(ndimage.convolve1d(x, g, axis=1, mode="nearest"), dg, axis=0, mode="nearest")
    return np.sqrt(gx ** 2 + gy ** 2)


def grad(pred, target, mask=None):
    e = (grad_amplitude(pred) - grad_amplitude(target)) ** 2
    return float((e if mask is None else e * (np.asarray(mask) != 0)).sum())


def largest_component(m):
    """Boolean map of the largest 4-connected component of m; among equal sizes the one whose first pixel comes first in
    raster order (skimage numbering + np.argmax).  None when m is empty."""
    lab, n = ndimage.label(m, structure=CROSS)
    if n == 0:
        return None
    size = np.bincount(lab.ravel())[1:]
    cand = np.flatnonzero(size == size.max()) + 1
    if len(cand) == 1:
        win = cand[0]
    else:                                               # tie: smallest first linear index, independent of the numbering
        flat = lab.ravel()
        idx = np.flatnonzero(np.isin(flat, cand))
        win = flat[idx[0]]
    return lab == win


def conn_level_map(pred, target):
    """uint8 [H,W]: k where the reference's l_map holds t_k (k = 0..9), 10 where it holds 1.0."""
    pred, target = np.asarray(pred, np.uint8), np.asarray(target, np.uint8)
    lev = np.full(pred.shape, 10, np.uint8)
    unset = np.ones(pred.shape, bool)
    for i, c in enumerate(cutoffs(), start=1):
        omega = largest_component((pred >= c) & (target >= c))
        flag = unset if omega is None else unset & ~omega
        lev[flag] = i - 1
        unset &= ~flag
    return lev


def conn_terms(pred, target, level_map):
    """Per-pixel |phi_p - phi_t| in float32, the reference's arithmetic (metric.py:228-233)."""
    lv = levels()[np.asarray(level_map)]
    th = np.float32(THETA)

    def phi(u8):
        d = np.asarray(u8, np.float32) / np.float32(255) - lv
        return np.float32(1) - d * (d >= th).astype(np.float32)
    return np.abs(phi(pred) - phi(target))


def conn(pred, target, mask=None):
    t = conn_terms(pred, target, conn_level_map(pred, target)).astype(np.float64)
    return float((t if mask is None else t * (np.asarray(mask) != 0)).sum())
