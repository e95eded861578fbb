"""Generate tests/golden/metrics_grad_conn.npz from the REFERENCE's own Grad and Conn (development container only).

    python -m tests.golden.make_metric_golden

Imports the reference's utils/tmp/metric.py through tools/ref_import.load_reference() and calls
BatchMetric.BatchGradient / BatchConnectivity on the CPU (the object is made with __new__ and CPU ImageFilters: its
__init__ moves them to CUDA).  skimage is not installed here, so skimage.measure.label is registered as a stand-in built
on scipy.ndimage.label with the 4-neighbour cross: both number components in raster order of their first pixel, which
is what findMaxConnectedRegion's np.argmax tie-break depends on.  Conn is therefore pinned "by definition" at that one
third-party boundary, as the cv2 stand-in does for the exact EDT.  The fixture holds data only.

Frames (uint8 pred / target / {0,1} mask, one frame per reference call):
  smooth random pairs; a checkerboard (every component has size 1: the tie-break decides); two equal-size blobs in both
  raster orders; a one-pixel-wide spiral; an empty mask, an all-255 and an all-0 frame; 1 x W and H x 1 strips; a frame
  of every cutoff neighbour (25/26, 50/51/52, ..., 254/255) on pred and target.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tools.ref_import import load_reference  # noqa: E402

H, W = 48, 64


def _skimage_standin():
    from scipy import ndimage
    sk = types.ModuleType("skimage")
    skm = types.ModuleType("skimage.measure")
    cross = ndimage.generate_binary_structure(2, 1)

    def label(x, connectivity=None, return_num=False):
        assert connectivity == 1
        lab, n = ndimage.label(np.asarray(x) != 0, structure=cross)
        return (lab, n) if return_num else lab
    skm.label = label
    sk.measure = skm
    sys.modules["skimage"] = sk
    sys.modules["skimage.measure"] = skm


def _smooth(rng, h, w, sigma):
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma, mode="wrap")
    f = (f - f.min()) / max(1e-12, f.max() - f.min())
    return f


def _unknown(t):
    return ((t > 0) & (t < 255)).astype(np.uint8)


def frames():
    rng = np.random.Generator(np.random.PCG64(2024))
    out = []
    for k in range(4):                                              # smooth random pairs
        a = _smooth(rng, H, W, 3.0 + k)
        t = np.clip(np.rint(a * 300 - 25), 0, 255).astype(np.uint8)
        p = np.clip(t.astype(np.int32) + np.rint(_smooth(rng, H, W, 2.0) * 60 - 30).astype(np.int32), 0, 255).astype(np.uint8)
        out.append(("smooth%d" % k, p, t, _unknown(t) if k % 2 == 0 else (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)))
    yy, xx = np.mgrid[:H, :W]
    chk = (yy + xx) % 2 == 0                                        # checkerboard: 4-connected components of size 1
    p = np.where(chk, rng.integers(30, 256, (H, W)), rng.integers(0, 26, (H, W))).astype(np.uint8)
    t = np.where(chk, rng.integers(30, 256, (H, W)), rng.integers(0, 26, (H, W))).astype(np.uint8)
    out.append(("checker", p, t, np.ones((H, W), np.uint8)))
    for order in range(2):                                          # two 8x8 blobs of equal size in both raster orders
        p = np.full((H, W), 10, np.uint8)
        t = np.full((H, W), 12, np.uint8)
        pos_a, pos_b = ((4, 44), (10, 6)) if order == 0 else ((10, 44), (4, 6))     # top-left corners (row, col)
        for (r, c), d in ((pos_a, 7), (pos_b, 20)):               # the loser's Conn term tells which blob won the tie
            p[r:r + 8, c:c + 8] = 200
            t[r:r + 8, c:c + 8] = 200 - d
        out.append(("blobs%d" % order, p, t, np.ones((H, W), np.uint8)))
    sp = np.zeros((H, W), bool)                                     # one-pixel-wide spiral, one path, turns two apart
    r, c, h, v = 1, 1, W - 3, H - 3
    sp[r, c] = True
    for j in range(4 * max(H, W)):
        L = h if j == 0 else (h if j % 2 == 0 else v) - 2 * ((j - 1) // 2)
        if L <= 0:
            break
        dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[j % 4]
        for _ in range(L):
            r, c = r + dr, c + dc
            sp[r, c] = True
    p = np.where(sp, 200, 20).astype(np.uint8)
    t = np.where(sp, 180 + rng.integers(0, 60, (H, W)), rng.integers(0, 40, (H, W))).astype(np.uint8)
    out.append(("spiral", p, t, np.ones((H, W), np.uint8)))
    a = _smooth(rng, H, W, 4.0)
    t = np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)
    out.append(("empty_mask", np.clip(t.astype(np.int32) + 9, 0, 255).astype(np.uint8), t, np.zeros((H, W), np.uint8)))
    out.append(("all255", np.full((H, W), 255, np.uint8), np.full((H, W), 255, np.uint8), np.ones((H, W), np.uint8)))
    out.append(("all0", np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)))
    s = np.clip(np.rint(_smooth(rng, 1, 97, 5.0) * 255), 0, 255).astype(np.uint8)
    out.append(("row_strip", s, np.clip(s.astype(np.int32) - 20, 0, 255).astype(np.uint8), np.ones((1, 97), np.uint8)))
    s = np.clip(np.rint(_smooth(rng, 83, 1, 5.0) * 255), 0, 255).astype(np.uint8)
    out.append(("col_strip", np.clip(s.astype(np.int32) + 15, 0, 255).astype(np.uint8), s, np.ones((83, 1), np.uint8)))
    vals = np.array([25, 26, 50, 51, 52, 101, 102, 152, 153, 203, 204, 229, 230, 254, 255], np.uint8)
    bp = rng.integers(0, len(vals), (H // 4, W // 4))                  # 4x4 blocks of one cutoff neighbour each
    bt = rng.integers(0, len(vals), (H // 4, W // 4))
    p = np.kron(vals[bp], np.ones((4, 4), np.uint8)).astype(np.uint8)
    t = np.kron(vals[bt], np.ones((4, 4), np.uint8)).astype(np.uint8)
    p[::7, ::5] = vals[rng.integers(0, len(vals), p[::7, ::5].shape)]   # and single pixels of them
    out.append(("cutoffs", p, t, np.ones((H, W), np.uint8)))
    return out


def main():
    load_reference()
    _skimage_standin()
    from utils.tmp.metric import BatchMetric, ImageFilter, genGaussKernel    # reference utils/tmp/metric.py
    bm = BatchMetric.__new__(BatchMetric)
    bm.conn_step, bm.conn_thresh, bm.conn_theta, bm.conn_p, bm.device = 0.1, 0.5, 0.15, 1, "cpu"
    hx, hy, size = genGaussKernel(1.4, 2)
    bm.hx, bm.hy, bm.kernel_size = hx, hy, size
    bm.fx = ImageFilter(1, size, torch.from_numpy(hx[::-1, ::-1].copy())[None, None], "cpu")
    bm.fy = ImageFilter(1, size, torch.from_numpy(hy[::-1, ::-1].copy())[None, None], "cpu")
    res = {}
    names, grads, conns = [], [], []
    for i, (name, p, t, m) in enumerate(frames()):
        pt = torch.from_numpy(p.astype(np.float32))[None]
        tt = torch.from_numpy(t.astype(np.float32))[None]
        mt = torch.from_numpy(m.astype(np.float32))[None]
        with torch.no_grad():
            grads.append(float(bm.BatchGradient(pt, tt, mt)[0]))
            conns.append(float(bm.BatchConnectivity(pt, tt, mt)[0]))
        res["pred_%d" % i], res["target_%d" % i], res["mask_%d" % i] = p, t, m
        names.append(name)
    res["names"] = np.array(names)
    res["grad"] = np.array(grads, np.float32)            # float32 values the reference returns
    res["conn"] = np.array(conns, np.float32)
    steps = torch.arange(0, 1 + 0.1, 0.1)               # metric.py:215 (float32, CPU)
    x = torch.arange(256).float() / 255.
    res["levels"] = steps.numpy()
    res["passes"] = np.stack([(x >= steps[i]).numpy() for i in range(1, len(steps))], 1)   # [256, 10] bool
    path = os.path.join(HERE, "metrics_grad_conn.npz")
    np.savez_compressed(path, **res)
    print("wrote %s (%d bytes): %s" % (path, os.path.getsize(path), ", ".join("%s %.6g/%.6g" % z for z in zip(names, grads, conns))))


if __name__ == "__main__":
    main()
