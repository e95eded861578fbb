"""Region-of-interest matting without a GPU: the restated box against brute force, the window policy on hand-worked cases, the
refusals that need no device, and the binding (header, lib.py and the built library carry the three symbols; ABI still 21)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import roi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restated box
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (7, 13), (12, 16)])
def test_restated_bbox_equals_brute_force(H, W):
    g = np.random.default_rng(100 * H + W)
    for trial in range(12):
        # one-hot maps, sparse enough that empty classes and single pixels occur
        cls = g.choice(3, size=(H, W), p=[(0.9, 0.05, 0.05), (0.4, 0.3, 0.3), (0.0, 0.5, 0.5), (1.0, 0.0, 0.0)][trial % 4])
        onehot = np.stack([(cls == k) for k in range(3)]).astype(np.float32)
        assert np.array_equal(R.bbox(onehot), R.bbox_brute(onehot)), (trial, "one-hot")
        # probabilities on a coarse grid: ties t1 == t2 and t0 == max(t1, t2) are common
        prob = (g.integers(0, 4, size=(3, H, W)) / 4.0).astype(np.float32)
        assert np.array_equal(R.bbox(prob), R.bbox_brute(prob)), (trial, "probabilities")
        lab = g.choice(np.array([0, 1, 2, 255, 7], np.uint8), size=(H, W), p=(0.6, 0.1, 0.1, 0.15, 0.05))
        assert np.array_equal(R.bbox(lab), R.bbox_brute(lab)), (trial, "labels")


def test_restated_bbox_on_hand_made_maps():
    t = np.zeros((3, 5, 7), np.float32)
    t[0] = 1
    assert R.bbox(t).tolist() == [5, 7, -1, -1, 5, 7, -1, -1]
    t[:, 2, 3] = (0.2, 0.4, 0.4)                            # t1 == t2 above t0: unknown
    t[:, 4, 6] = (0.5, 0.5, 0.1)                            # t0 == max(t1, t2): background
    t[:, 0, 1] = (0.1, 0.2, 0.7)                            # foreground: non-bg only
    assert R.bbox(t).tolist() == [2, 3, 2, 3, 0, 1, 2, 3]
    lab = np.full((4, 4), 255, np.uint8)
    lab[1, 2], lab[3, 0] = 2, 1
    assert R.bbox(lab).tolist() == [3, 0, 3, 0, 1, 0, 3, 2]


# ------------------------------------------------------------------ the window policy
def test_window_size_and_origin_hand_worked():
    from otvm_amd import roi
    H, W = 400, 600
    assert roi.ALIGN == 32
    # exactly 64 rows with margin 0 stay 64; 65 rows need 96
    assert roi.window_size([(10, 20, 73, 83)], H, W, 0) == (64, 64)
    assert roi.window_size([(10, 20, 74, 84)], H, W, 0) == (96, 96)
    assert roi.window_size([(10, 20, 73, 83)], H, W, 1) == (96, 96)
    assert roi.window_size([(10, 20, 41, 51), (H, W, -1, -1), (0, 0, 9, 99)], H, W, 16) == (64, 160)     # the largest extents
    # a need above the frame's side gives the side itself (also one that is no multiple of 32)
    assert roi.window_size([(0, 0, 389, 10)], H, W, 0) == (400, 32)
    assert roi.window_size([(0, 0, 10, 590)], H, W, 8) == (32, 600)
    assert roi.window_size([(5, 5, 5, 5)], 20, 50, 0) == (20, 32)
    # no non-empty box at all
    assert roi.window_size([], H, W, 32) == (32, 32) and roi.window_size([(H, W, -1, -1)], H, W, 32) == (32, 32)
    assert roi.window_size([], 20, 50, 0) == (20, 32)
    # centred: (y0 + y1 + 1) // 2 - h // 2
    assert roi.window_origin((100, 200, 163, 263), 64, 64, H, W) == (100, 200)
    assert roi.window_origin((100, 200, 120, 221), 64, 96, H, W) == ((100 + 120 + 1) // 2 - 32, (200 + 221 + 1) // 2 - 48)
    # clamped at the top, the left, the bottom and the right side of the frame
    assert roi.window_origin((0, 300, 10, 310), 64, 64, H, W) == (0, 273)
    assert roi.window_origin((200, 2, 210, 8), 64, 64, H, W) == (173, 0)
    assert roi.window_origin((390, 300, 399, 310), 64, 64, H, W) == (336, 273)
    assert roi.window_origin((200, 590, 210, 599), 64, 64, H, W) == (173, 536)
    # an empty box keeps the previous origin; the first frame's is (0, 0)
    assert roi.window_origin((H, W, -1, -1), 64, 64, H, W, (17, 33)) == (17, 33)
    assert roi.window_origin((H, W, -1, -1), 64, 64, H, W) == (0, 0)
    # the restatement the GPU tests predict windows with says the same
    g = np.random.default_rng(3)
    for _ in range(200):
        y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
        box = (y0, x0, int(g.integers(y0, H)), int(g.integers(x0, W)))
        margin = int(g.integers(0, 40))
        h, w = roi.window_size([box], H, W, margin)
        assert (h, w) == R.window_size([box], H, W, margin) and (h % 32 == 0 or h == H) and (w % 32 == 0 or w == W)
        at = roi.window_origin(box, h, w, H, W)
        assert at == R.window_origin(box, h, w, H, W) and 0 <= at[0] <= H - h and 0 <= at[1] <= W - w
        if box[2] - box[0] + 1 <= h and box[3] - box[1] + 1 <= w:
            assert roi.contains(at + (h, w), box)


def test_contains_union_and_touched_sides():
    from otvm_amd import roi
    win = (10, 20, 64, 96)                                   # rows 10 ... 73, columns 20 ... 115
    assert roi.contains(win, (10, 20, 73, 115))              # touching all four sides from inside
    for out in ((9, 20, 73, 115), (10, 19, 73, 115), (10, 20, 74, 115), (10, 20, 73, 116)):
        assert not roi.contains(win, out)
    assert roi.contains(win, (200, 300, -1, -1))             # an empty box lies in every window
    assert roi.union([(5, 5, -1, -1)]) is None and roi.union([(3, 9, 4, 10), (50, 60, -1, -1), (1, 20, 2, 30)]) == (1, 9, 4, 30)
    H, W = 200, 300
    assert not roi.touched_sides(win, (11, 21, 72, 114), H, W)
    for box in ((10, 50, 20, 60), (30, 20, 40, 30), (60, 50, 73, 60), (30, 100, 40, 115)):
        assert roi.touched_sides(win, box, H, W), box
    # a side of the window that is the frame's own side does not count
    assert not roi.touched_sides((0, 0, 64, 96), (0, 0, 20, 20), H, W)
    assert not roi.touched_sides((136, 204, 64, 96), (180, 280, 199, 299), H, W)
    assert roi.touched_sides((136, 204, 64, 96), (136, 280, 199, 299), H, W)


def test_check_window_refusals():
    from otvm_amd import roi
    assert roi.check_window((0, 0, 10, 20), 10, 20) == (0, 0, 10, 20)
    assert roi.check_window([3, 4, np.int64(5), 6], 10, 20) == (3, 4, 5, 6)
    for bad, word in (((0, 0, 0, 5), "empty"), ((0, 0, 5, 0), "empty"), ((-1, 0, 5, 5), "leaves"), ((0, -1, 5, 5), "leaves"),
                      ((6, 0, 5, 5), "leaves"), ((0, 16, 5, 5), "leaves"), ((0, 0, 11, 5), "leaves"), ((0, 0, 5, 21), "leaves"),
                      ((0, 0, 5), "four integers"), ("auto", "four integers"), ((0, 0, 5.5, 5), "four integers"), (None, "four integers")):
        with pytest.raises(ValueError, match=word):
            roi.check_window(bad, 10, 20)
    with pytest.raises(ValueError, match="10x20"):
        roi.check_window((0, 0, 11, 5), 10, 20)


# ------------------------------------------------------------------ refusals that need no device
class _NoDevice(torch.nn.Module):
    DILATION_KERNEL = 12

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_clip_plan_refusals_need_no_device():
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    model = _NoDevice()
    H, W, T = 40, 48, 3
    frames = [np.zeros((H, W, 3), np.uint8)] * T
    m = np.zeros((H, W), np.uint8)
    tri = np.zeros((3, H, W), np.float32)
    for kw, word in ((dict(roi="auto", trimap=tri, work_scale=2), "work_scale"),
                     (dict(roi="auto", alphas=[m] * T), "alphas"),
                     (dict(roi="auto", trimap=tri, backgrounds=frames), "backgrounds"),
                     (dict(roi="window", trimap=tri), "'auto'"),
                     (dict(roi=(0, 0, 32), trimap=tri), "four integers"),
                     (dict(roi=(0, 0, 32.5, 32), trimap=tri), "four integers"),
                     (dict(roi=(0, 0, 0, 32), trimap=tri), "h, w >= 1"),
                     (dict(roi=(-1, 0, 32, 32), trimap=tri), "y0, x0 >= 0"),
                     (dict(roi=(16, 0, 32, 32), trimap=tri), "leaves the 40x48 frame"),
                     (dict(roi=(0, 32, 32, 32), masks=[m] * T), "leaves the 40x48 frame"),
                     (dict(roi="auto", roi_margin=-1, trimap=tri), "roi_margin"),
                     (dict(roi="auto", roi_margin=2.5, trimap=tri), "roi_margin"),
                     (dict(roi="auto"), "trimap flow")):
        with pytest.raises(ValueError, match=word):
            run_video_matte(model, frames, **kw)
    with pytest.raises(ValueError, match="float frames"):
        run_video_matte(model, [f.astype(np.float32) for f in frames], trimap=tri, roi="auto")
    with pytest.raises(ValueError, match="single-clip"):
        run_video_matte_batch(model, [frames], trimaps=[tri], roi="auto")
    # the refusals of the other options come as before
    with pytest.raises(ValueError, match="one mask per frame"):
        run_video_matte(model, frames, masks=[m] * 2, roi="auto")


def test_eval_cli_refuses_roi_outside_its_route(tmp_path):
    from otvm_amd import eval_cli
    data = str(tmp_path)
    for argv, word in ((["--roi", "auto"], "--demo"), (["--demo", "--roi", "auto", "--work-scale", "2"], "--work-scale"),
                       (["--demo", "--roi", "auto", "--viz"], "--viz"), (["--demo", "--roi", "auto", "--batch", "2"], "--batch"),
                       (["--demo", "--roi", "1,2,3"], "--roi"), (["--demo", "--roi", "0,0,0,5"], "--roi"),
                       (["--demo", "--roi", "box"], "--roi"), (["--demo", "--roi", "auto", "--roi-margin", "-4"], "--roi-margin"),
                       (["--demo", "--roi-margin", "4"], "--roi-margin")):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(["--data", data, "--synthetic-weights"] + argv)
        assert word in str(e.value), (argv, str(e.value))
    assert eval_cli.parse_roi_options("auto", None) == ("auto", 32)
    assert eval_cli.parse_roi_options("4,8,64,96", 5) == ((4, 8, 64, 96), 5)
    assert eval_cli.parse_roi_options(None, None) == (None, 32)


# ------------------------------------------------------------------ the binding
def _struct_fields(header, name):
    body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl)
            names += [n.strip().lstrip("*") for n in decl.split(",")]
    return names


def test_binding_declares_the_roi_entry_points():
    import __graft_entry__ as g
    from otvm_amd import lib as L
    from otvm_amd.csrc import build as B
    h = ctypes.CDLL(g.build())
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    for sym in ("otvm_trimap_bbox", "otvm_roi_crop", "otvm_roi_paste"):
        assert sym in L.EXPORTED and getattr(h, sym) is not None
        assert re.search(r"\bint %s\(const \w+\* p, void\* stream\);" % sym, header), sym
    assert ("roi.hip", ["-ffp-contract=off"]) in B.SOURCES
    h.otvm_abi_version.restype = ctypes.c_int
    assert h.otvm_abi_version() == 21 == L.ABI_VERSION and "#define OTVM_ABI_VERSION 21 " in header
    for cname, cls, size in (("otvm_roi_bbox_params", L.RoiBboxParams, 32), ("otvm_roi_crop_params", L.RoiCropParams, 72),
                             ("otvm_roi_paste_params", L.RoiPasteParams, 104)):
        assert _struct_fields(header, cname) == [f for f, _ in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname


def test_bad_arguments_are_refused_before_any_launch():
    """The checks precede the launch, so they answer without a device: nonzero, and the message starts with the function's name."""
    import __graft_entry__ as g
    from otvm_amd import lib as L
    g.build()
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    at = ctypes.addressof(buf)

    def refused(fn, p, name):
        assert fn(ctypes.byref(p), None) != 0
        assert lib.otvm_last_error().decode().startswith(name + ":"), lib.otvm_last_error()

    for kw in (dict(), dict(trimap=at, labels=at), dict(trimap=at, H=0, W=5), dict(labels=at, H=5, W=16384), dict(labels=at, H=16384, W=5),
               dict(labels=at, H=-2, W=5)):
        p = L.RoiBboxParams()
        p.H, p.W, p.out = 4, 4, at
        for k, v in kw.items():
            setattr(p, k, v)
        refused(lib.otvm_trimap_bbox, p, "otvm_trimap_bbox")
    p = L.RoiBboxParams()
    p.H, p.W, p.labels = 4, 4, at
    refused(lib.otvm_trimap_bbox, p, "otvm_trimap_bbox")                 # no out
    windows = (dict(h=0), dict(w=0), dict(y0=-1), dict(x0=-1), dict(y0=5), dict(x0=9), dict(h=9), dict(w=13), dict(H=0), dict(W=0),
               dict(H=16384), dict(W=16384), dict(y0=2 ** 31 - 1), dict(h=2 ** 31 - 1))
    for kw in windows + (dict(frame_out=None), dict(frame=None)):
        p = L.RoiCropParams()
        p.H, p.W, p.y0, p.x0, p.h, p.w, p.frame, p.frame_out = 8, 12, 1, 1, 4, 4, at, at
        for k, v in kw.items():
            setattr(p, k, v)
        refused(lib.otvm_roi_crop, p, "otvm_roi_crop")
    for kw in windows + (dict(alpha=None), dict(win_alpha=None), dict(win_trimap=None), dict(fgr=at), dict(fgr=at, win_fgr=at),
                         dict(fgr=at, frame=at)):
        p = L.RoiPasteParams()
        p.H, p.W, p.y0, p.x0, p.h, p.w, p.win_alpha, p.win_trimap, p.alpha = 8, 12, 1, 1, 4, 4, at, at, at
        for k, v in kw.items():
            setattr(p, k, v)
        refused(lib.otvm_roi_paste, p, "otvm_roi_paste")
