"""Working-resolution matting, host side (no GPU): the library's new symbols, the numpy restatement's reduction rules on
hand-written cases, its two properties (solid regions stay exact, a sub-pixel edge beats bilinear), and the drivers' arguments."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import guided_cases as K
from tests import guided_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("otvm_downsample_u8", "otvm_downsample_trimap", "otvm_downsample_labels", "otvm_guided_ws_bytes", "otvm_guided_coeffs",
           "otvm_guided_apply")


def test_library_exports_guided_symbols_and_keeps_abi_21(tmp_path):
    from otvm_amd.csrc.build import build
    from otvm_amd import lib as L
    build()
    h = L.load()
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    for sym in SYMBOLS:
        assert sym in L.EXPORTED and getattr(h, sym) is not None
        assert (" " + sym + "(") in header, sym
    assert "typedef struct otvm_guided_params" in header
    assert h.otvm_abi_version() == 21 and L.ABI_VERSION == 21 and "#define OTVM_ABI_VERSION 21" in header
    src = '#include <stdio.h>\n#include "otvm_hip.h"\nint main(){printf("%zu %zu\\n", sizeof(otvm_guided_params), sizeof(otvm_fgr_params));return 0;}\n'
    exe = os.path.join(str(tmp_path), "guided_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    a, b = (int(v) for v in subprocess.check_output([exe]).split())
    assert ctypes.sizeof(L.GuidedParams) == a
    assert ctypes.sizeof(L.FgrParams) == b               # untouched by this feature
    assert h.otvm_guided_ws_bytes(5, 7, 4) == 5 * 7 * 4 * 16 and h.otvm_guided_ws_bytes(5, 7, 2) == -1
    # argument checks need no device: they fail before any launch
    p = L.GuidedParams()
    assert h.otvm_guided_coeffs(ctypes.byref(p), None, None) != 0 and h.otvm_guided_apply(ctypes.byref(p), None) != 0
    assert h.otvm_downsample_u8(None, 4, 4, 2, None, None) != 0


# ------------------------------------------------------------------------------------------------ reductions, 5 x 7 by hand
def test_downsample_u8_hand_cases():
    img = np.zeros((5, 7, 3), np.uint8)
    img[..., 0] = np.arange(35).reshape(5, 7)            # channel 0: 0..34
    img[..., 1] = 255
    img[0, 0, 2], img[0, 1, 2], img[1, 0, 2], img[1, 1, 2] = 1, 2, 2, 1     # sum 6 -> (6 + 2) // 4 = 2; 1, 1, 1, 2 would be 1
    out = R.downsample_u8(img, 2)
    assert out.shape == (3, 4, 3) and (out[..., 1] == 255).all()
    assert out[0, 0, 0] == (0 + 1 + 7 + 8 + 2) // 4                          # 18 // 4 = 4 (mean 4.0)
    assert out[0, 0, 2] == 2
    assert out[0, 3, 0] == (6 + 13 + 1) // 2                                 # right edge: a 2 x 1 block, 19/2 = 9.5 -> 10
    assert out[2, 0, 0] == (28 + 29 + 1) // 2                                # bottom edge: a 1 x 2 block, 28.5 -> 29
    assert out[2, 3, 0] == 34                                                # the corner: one pixel
    img2 = img.copy(); img2[:2, :2, 2] = [[1, 1], [1, 2]]
    assert R.downsample_u8(img2, 2)[0, 0, 2] == 1                            # 5 / 4 = 1.25 -> 1
    out3 = R.downsample_u8(img, 3)
    assert out3.shape == (2, 3, 3) and out3[1, 2, 0] == (27 + 34 + 1) // 2   # 2 x 1 corner block of s = 3
    assert out3[0, 0, 0] == (0 + 1 + 2 + 7 + 8 + 9 + 14 + 15 + 16 + 4) // 9
    out4 = R.downsample_u8(img, 4)
    assert out4.shape == (2, 2, 3) and out4[1, 1, 0] == (32 + 33 + 34 + 1) // 3


def test_downsample_trimap_hand_cases():
    cls = np.array([[2, 2, 2, 1, 0, 0, 0],
                    [2, 2, 2, 2, 0, 0, 0],
                    [2, 2, 0, 0, 0, 0, 1],
                    [2, 2, 0, 0, 0, 0, 0],
                    [2, 1, 0, 0, 2, 0, 0]])
    tri = np.stack([(cls == k) for k in range(3)]).astype(np.float32)
    out = R.downsample_trimap(tri, 2)
    want = np.array([[2, 1, 0, 0],
                     [2, 0, 0, 1],
                     [1, 0, 1, 0]])                       # mixed fg / bg blocks are unknown; the edge blocks use what exists
    assert np.array_equal(out.argmax(0), want) and np.array_equal(out.sum(0), np.ones((3, 4), np.float32))
    assert set(np.unique(out)) == {0.0, 1.0}
    # a soft (not exactly one) foreground never counts as solid
    soft = tri.copy(); soft[2, 0, 0] = np.float32(0.999)
    assert R.downsample_trimap(soft, 2).argmax(0)[0, 0] == 1
    # the unknown band never shrinks: every unknown pixel lands in an unknown block
    for s in (2, 3, 4):
        o = R.downsample_trimap(tri, s).argmax(0)
        ys, xs = np.nonzero(cls == 1)
        assert (o[ys // s, xs // s] == 1).all()


def test_downsample_labels_hand_cases():
    lab = np.array([[0, 0, 2, 2, 255, 0, 1],
                    [0, 0, 2, 1, 0, 0, 1],
                    [2, 0, 255, 255, 1, 1, 2],
                    [0, 2, 255, 255, 1, 1, 2],
                    [7, 0, 2, 2, 0, 1, 255]], np.uint8)
    out = R.downsample_labels(lab, 2)
    want = np.array([[0, 1, 255, 1],
                     [1, 255, 1, 2],
                     [255, 2, 1, 255]], np.uint8)        # 7 is no class: unlabelled, like 255
    assert np.array_equal(out, want)
    assert np.array_equal(R.downsample_labels(lab, 4), np.array([[255, 255], [255, 255]], np.uint8))
    assert np.array_equal(R.downsample_labels(np.full((5, 7), 2, np.uint8), 3), np.full((2, 3), 2, np.uint8))


# ------------------------------------------------------------------------------------------------ properties
def test_constant_target_gives_exact_coefficients():
    g = np.random.default_rng(1).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    g[:4, :5] = 17                                        # a constant region: eps alone conditions the solve
    for v in (0.0, 1.0, 0.25):
        raw, mean = R.guided_coeffs(g, [np.full((9, 11), v, np.float32)], 2, 1e-6)
        P = int(R.quantise(np.float32(v)))
        for c in (raw, mean):
            assert (c[..., :3] == 0).all() and (c[..., 3] == np.float32(np.float64(P) / 65535.0)).all()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_restatement_keeps_solid_regions(s):
    """The mean coefficients at a working pixel average the coefficients of the pixels within r, each of which looks at the
    target within r of itself: the filter's support is 2r.  So: wherever every working pixel within 2r of the four bilinear
    neighbours has target exactly 0 (1), the output is exactly 0.0 (1.0).  (Within r alone the statement is false for this
    filter, whatever the implementation: the restatement itself leaves hundreds of such pixels inexact on this input.)"""
    frame, wf, al = K.solid_case(s=s)
    H, W = frame.shape[:2]
    for r in (1, 2, 4):
        a, u8, _ = R.guided_upsample(frame, wf, [al], s, r, 1e-4)
        for v in (0.0, 1.0):
            m = K.solid_mask(al, v, H, W, s, 2 * r)
            assert m.sum() > 300, "the case has no solid region left"
            assert (a[m] == np.float32(v)).all() and (u8[m] == int(v * 255)).all()


def test_restatement_beats_bilinear_on_a_subpixel_edge():
    lines = []
    for s in (2, 3, 4):
        frame, true, wf, wa = K.edge_case(s=s)
        H, W = true.shape
        a, _, _ = R.guided_upsample(frame, wf, [wa], s, 2, 1e-4)
        b = R.bilinear_upsample(wa, H, W, s)
        sg, sb = float(np.abs(a - true).sum()), float(np.abs(b - true).sum())
        lines.append("s=%d r=2 eps=1e-4: guided SAD %.3f, bilinear SAD %.3f, ratio %.3f" % (s, sg, sb, sg / sb))
        assert sg < sb
    print("\n".join(lines))


# ------------------------------------------------------------------------------------------------ drivers
class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.foreground, self._background = False, None

    def forward(self, *a, **k):
        raise AssertionError("the model must not run: the arguments are refused first")


def test_run_video_matte_refuses_what_the_working_route_cannot_do():
    from otvm_amd import video
    sig = inspect.signature(video.run_video_matte)
    assert sig.parameters["work_scale"].default is None and sig.parameters["work_radius"].default == 2
    assert sig.parameters["work_eps"].default == 1e-4 and sig.parameters["on_foreground"].default is None
    assert "PLACEHOLDERS" in video.run_video_matte.__doc__
    m, cpu = _Stub(), torch.device("cpu")
    u8 = [np.zeros((8, 12, 3), np.uint8)] * 2
    tri = np.zeros((3, 8, 12), np.float32); tri[1] = 1
    kw = dict(device=cpu)
    with pytest.raises(ValueError, match="work_scale is 2, 3 or 4"):
        video.run_video_matte(m, u8, trimap=tri, work_scale=5, **kw)
    with pytest.raises(ValueError, match="work_scale is 2, 3 or 4"):
        video.run_video_matte(m, u8, trimap=tri, work_scale=1.5, **kw)
    for r in (0, 5):
        with pytest.raises(ValueError, match="work_radius is 1 ... 4"):
            video.run_video_matte(m, u8, trimap=tri, work_scale=2, work_radius=r, **kw)
    with pytest.raises(ValueError, match="alphas flow"):
        video.run_video_matte(m, u8, alphas=[np.zeros((8, 12), np.float32)] * 2, work_scale=2, **kw)
    with pytest.raises(ValueError, match="float frames"):
        video.run_video_matte(m, [np.zeros((8, 12, 3), np.float32)] * 2, trimap=tri, work_scale=2, **kw)
    with pytest.raises(ValueError, match="single-clip"):
        video.run_video_matte_batch(m, [u8], trimaps=[tri], work_scale=2, **kw)


def test_eval_cli_has_the_working_resolution_options(monkeypatch):
    import argparse
    from otvm_amd import eval_cli
    seen = {}

    class Stop(Exception):
        pass
    orig = argparse.ArgumentParser.parse_args

    def spy(self, argv=None):
        ns = orig(self, argv)
        seen.update(vars(ns))
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(Stop):
        eval_cli.main(["--demo", "--data", "x", "--work-scale", "3", "--work-radius", "1", "--work-eps", "0.01"])
    assert seen["work_scale"] == 3 and seen["work_radius"] == 1 and seen["work_eps"] == 0.01
    with pytest.raises(Stop):
        eval_cli.main(["--demo", "--data", "x"])
    assert seen["work_scale"] is None
