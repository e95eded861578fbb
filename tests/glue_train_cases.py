"""Shapes and inputs shared by tests/test_glue_train_cpu.py (the yardstick) and tests/test_gpu_glue.py / tests/test_gpu_train.py (the
kernels): the smallest sizes that reach each branch of csrc/glue.hip and csrc/losses.hip.  The caps: glue.hip's grid_for launches at
most 8192 x 256 = 2,097,152 threads, losses.hip's lgrid 2048 x 256 = 524,288, its exclusion kernels 64 x 256 = 16,384 per image."""
import numpy as np
import torch

GLUE_CAP, LOSS_CAP, EXCL_CAP = 8192 * 256, 2048 * 256, 64 * 256

# (H, W, Hp, Wp, lh, lw); the last is above GLUE_CAP
PREPROCESS = [(50, 70, 64, 96, 7, 13), (5, 7, 32, 32, 0, 25), (64, 96, 64, 96, 0, 0), (1050, 2040, 1056, 2048, 3, 4)]
# (h4, w4, ld); the last has 2,106,368 outputs
UPSAMPLE = [(1, 1, 4), (1, 5, 4), (3, 1, 8), (5, 7, 4), (17, 30, 4), (272, 484, 4)]
TRIMAP_TO_SM = [35, 2100000]
HEAD_P = [37 * 41, 1040 * 2020]                                  # 2,100,800 > GLUE_CAP

# (B, S, H, W)
STREAM = [(1, 1, 4, 6), (2, 3, 5, 7), (1, 2, 512, 544)]          # fba_comp, grad_l1, ce3, temporal: the last has 557,056 pixels
EXCLUSION = [(1, 1, 2, 2), (2, 3, 5, 1), (1, 2, 1, 7), (2, 3, 64, 96), (1, 2, 136, 128)]     # the last: 17,408 pixels per image
# (N, H, W): 4 x 4 reflects on both sides of every pixel; 6 x 288 x 320 = 552,960 pixels is above LOSS_CAP for the diff kernel (its
# down kernels have 138,240 outputs), 6 x 592 x 592 is above it for the down kernels too (525,696 outputs)
LAP = [(1, 4, 4), (3, 4, 6), (2, 6, 4), (5, 64, 96), (6, 288, 320), (6, 592, 592)]
AVGPOOL = [(1, 2, 2), (3, 6, 10), (3, 512, 1376)]                # the last: 528,384 outputs
FBA_LOSS = [(1, 1, 64, 64), (2, 3, 64, 96), (1, 2, 512, 544)]

assert PREPROCESS[-1][2] * PREPROCESS[-1][3] > GLUE_CAP and 16 * UPSAMPLE[-1][0] * UPSAMPLE[-1][1] > GLUE_CAP
assert TRIMAP_TO_SM[-1] > GLUE_CAP and HEAD_P[-1] > GLUE_CAP
assert STREAM[-1][1] * STREAM[-1][2] * STREAM[-1][3] > LOSS_CAP and EXCLUSION[-1][2] * EXCLUSION[-1][3] > EXCL_CAP
assert LAP[-2][0] * LAP[-2][1] * LAP[-2][2] > LOSS_CAP and LAP[-1][0] * LAP[-1][1] * LAP[-1][2] // 4 > LOSS_CAP and AVGPOOL[-1][0] * AVGPOOL[-1][1] * AVGPOOL[-1][2] // 4 > LOSS_CAP


def ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def preprocess_inputs(H, W, seed):
    """a float32 [H, W] with exact 0 / 1 regions; fg / bg uint8 [H, W, 3] in BGR order (every byte value occurs)."""
    g = np.random.default_rng(seed)
    a = g.random((H, W), dtype=np.float32)
    a[a < 0.2] = 0.0
    a[a > 0.8] = 1.0
    fg = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bg = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    fg[0, :min(W, 256), 0] = np.arange(min(W, 256))
    return a, fg, bg


def planes_f32(u8):
    """uint8 [H, W, 3] -> float32 planes [3, H, W] in the same channel order: what the caller's .float() gives."""
    return np.ascontiguousarray(u8.transpose(2, 0, 1).astype(np.float32))


def logits(h4, w4, scale, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((3, h4, w4)) * scale).astype(np.float32)


def loss_inputs(B, S, H, W, seed=3):
    """Uniform-random pred7 [B,S,7,H,W], gts clipped to exact 0 / 1, a 0 / 1 trimask, fgs / bgs / imgs [B,S,3,H,W]."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, S, 7, H, W, generator=g)
    gts = torch.rand(B, S, 1, H, W, generator=g)
    gts[gts < 0.3] = 0.0
    gts[gts > 0.8] = 1.0
    tm = (torch.rand(B, S, 1, H, W, generator=g) > 0.5).float()
    fgs, bgs, imgs = (torch.rand(B, S, 3, H, W, generator=g) for _ in range(3))
    return pred, gts, tm, fgs, bgs, imgs


def pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)
