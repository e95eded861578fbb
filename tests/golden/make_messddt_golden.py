"""Generate tests/golden/metrics_messddt.npz from the REFERENCE's own MESSDdt (development container only).

    python -m tests.golden.make_messddt_golden

Imports the reference's utils/tmp/metric.py through tools/ref_import.load_reference(), whose cv2 stand-in answers
calcOpticalFlowFarneback with the restatement of tests/farneback_ref.py (float32, the reference's fixed arguments asserted),
and calls BatchMetric.MESSDdt on the CPU, once with float32 tensors and once with float64.  The reference's Pool is replaced
by a serial map.  Each pair (i, i+1) is one two-frame call: torch.take (metric.py:295-297) indexes the flattened batch, so in
a longer batch every pair would read its warped values from the batch's second frame.

This pins the warp (the transposed lookup), the rounding and the sums to the reference's code.  It does not pin the flow:
the flow is the restatement's, checked against cv2 by definition only.  The fixture holds data only.

Clips (uint8 pred / target, default mask 0 < target < 255): soft blobs moving by whole and sub-pixel offsets with some
deformation, at sizes with 1, 2, 3 and 4 pyramid levels (level counts 0 .. 3), one of them non-square; one clip without
motion.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tools.ref_import import load_reference  # noqa: E402
from tests import farneback_ref as F  # noqa: E402


def blob_frame(H, W, blobs):
    """uint8 alpha of soft elliptic blobs [(cy, cx, ry, rx, edge)]."""
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    a = np.zeros((H, W))
    for cy, cx, ry, rx, edge in blobs:
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        a = np.maximum(a, np.clip((1.0 - d) * min(ry, rx) / edge + 0.5, 0, 1))
    return np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)


def moving_clip(rng, H, W, T, step, nblobs=2):
    blobs = []
    for _ in range(nblobs):
        blobs.append([rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.12, 0.22) * H,
                      rng.uniform(0.12, 0.22) * W, rng.uniform(3, 8)])
    tgt = []
    for t in range(T):
        tgt.append(blob_frame(H, W, blobs))
        for b in blobs:
            b[0] += step[0] + rng.uniform(-0.4, 0.4)
            b[1] += step[1] + rng.uniform(-0.4, 0.4)
            b[2] *= rng.uniform(0.97, 1.03)
            b[3] *= rng.uniform(0.97, 1.03)
    return np.stack(tgt)


def predict(rng, tgt):
    """pred = target with a smooth perturbation, clipped."""
    from scipy import ndimage
    noise = ndimage.gaussian_filter(rng.standard_normal(tgt.shape), (0, 2, 2)) * 120
    return np.clip(tgt.astype(np.float64) + noise, 0, 255).astype(np.uint8)


def clips():
    rng = np.random.Generator(np.random.PCG64(2026))
    out = []
    t = moving_clip(rng, 40, 56, 3, (1.6, -2.3))                       # 1 level, non-square
    out.append(("nonsq_l0", predict(rng, t), t))
    t0 = moving_clip(rng, 48, 64, 1, (0, 0))[0]
    t = np.stack([t0, t0, t0])                                         # zero motion
    out.append(("still", predict(rng, t), t))
    t = moving_clip(rng, 72, 96, 3, (-2.5, 3.2))                       # 2 levels
    out.append(("l1", predict(rng, t), t))
    t = moving_clip(rng, 136, 160, 2, (4.3, 1.7), nblobs=3)            # 3 levels
    out.append(("l2", predict(rng, t), t))
    t = moving_clip(rng, 264, 256, 2, (2.2, -5.4), nblobs=3)           # 4 levels
    out.append(("l3", predict(rng, t), t))
    return out


def main():
    load_reference()
    from tests.golden.make_metric_golden import _skimage_standin
    _skimage_standin()                                                 # metric.py imports skimage (unused by MESSDdt)
    import utils.tmp.metric as metric                                 # reference utils/tmp/metric.py

    class SerialPool:
        def __init__(self, n):
            pass

        def imap(self, f, items):
            return map(f, items)

        def close(self):
            pass
    metric.Pool = SerialPool
    bm = metric.BatchMetric.__new__(metric.BatchMetric)
    bm.device = "cpu"
    res = {}
    names = []
    for ci, (name, p, t) in enumerate(clips()):
        m = F.unknown_mask(t)
        e32, n32, e64, n64, flows, share = [], [], [], [], [], []
        for i in range(len(t) - 1):
            for dt, e, n in ((torch.float32, e32, n32), (torch.float64, e64, n64)):
                pt = torch.from_numpy(p[i:i + 2].astype(np.float64)).to(dt)
                tt = torch.from_numpy(t[i:i + 2].astype(np.float64)).to(dt)
                mt = torch.from_numpy(m[i:i + 2].astype(np.float64)).to(dt)
                err, num = bm.MESSDdt(pt, tt, mt)
                e.append(float(err[0]))
                n.append(float(num[0]))
            f32 = F.farneback(t[i], t[i + 1], np.float32)
            f64 = F.farneback(t[i], t[i + 1], np.float64)
            flows.append(F.rint_flow(f32).astype(np.int16))
            tol = max(3 * float(np.abs(f32.astype(np.float64) - f64).max()), 1e-4)
            amb = np.abs(np.abs(f64 - np.floor(f64)) - 0.5) <= tol
            share.append([float(amb[..., 0].mean()), float(amb[..., 1].mean())])
        res["pred_%d" % ci], res["target_%d" % ci] = p, t
        res["err32_%d" % ci], res["num32_%d" % ci] = np.array(e32, np.float32), np.array(n32, np.float32)
        res["err64_%d" % ci], res["num64_%d" % ci] = np.array(e64), np.array(n64)
        res["flow_%d" % ci] = np.stack(flows)
        names.append(name)
        print("%-9s %s  levels %d  err64 %s  ambiguous share %s" % (name, t.shape, len(F.level_table(*t.shape[1:])),
                                                                   np.round(e64, 6), np.round(share, 5)))
    res["names"] = np.array(names)
    path = os.path.join(HERE, "metrics_messddt.npz")
    np.savez_compressed(path, **res)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
