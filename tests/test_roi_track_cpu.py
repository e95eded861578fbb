"""The tracking window of region-of-interest matting without a GPU: the host policy (otvm_amd.roi.track_origin) against its
restatement (tests/roi_track_ref.py) on an exhaustive small grid and on the edge cases, the binding of the three new entry points
(refusals before any launch, the new struct's size, ABI still 21), and the refusals of run_video_matte(roi="track")."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import roi_track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the policy
def test_track_origin_equals_the_restatement_on_every_case_of_a_small_grid():
    """Every box of a 12x14 frame, a 5x6 window at every legal origin (and none), hold 1, 2, 3: every case of each axis, and a
    seeded subset of the cross product of the two."""
    from otvm_amd import roi
    H, W, h, w = 12, 14, 5, 6
    boxes = [(y0, x0, y1, x1) for y0 in range(H) for y1 in range(y0, H) for x0 in range(W) for x1 in range(x0, W)]
    boxes.append((H, W, -1, -1))
    origins = [(oy, ox) for oy in range(H - h + 1) for ox in range(W - w + 1)]
    n = 0
    # the cross product is 8191 boxes x 72 origins x 3 holds = 1.8 million calls of two functions: too slow.  An axis of the
    # result depends on that axis of the box and the origin alone (asserted below), so every y case is paired with two x cases
    # instead: every case of each axis occurs, held and recentred in every combination.
    ys = [(y0, y1, oy) for y0 in range(H) for y1 in range(y0, H) for oy in range(H - h + 1)]
    xs = [(x0, x1, ox) for x0 in range(W) for x1 in range(x0, W) for ox in range(W - w + 1)]
    for hold in (1, 2, 3):
        for i in range(max(len(ys), len(xs))):
            for j in (i, 7 * i + 3):
                (y0, y1, oy), (x0, x1, ox) = ys[i % len(ys)], xs[j % len(xs)]
                box, prev = (y0, x0, y1, x1), (oy, ox)
                assert roi.track_origin(box, prev, h, w, H, W, hold) == TR.track_origin(box, prev, h, w, H, W, hold), (box, prev, hold)
                n += 1
    # the full function on a seeded subset of the cross product, and on every box with no previous origin
    g = np.random.default_rng(12)
    for k in g.integers(0, len(boxes), size=20000):
        box, prev, hold = boxes[int(k)], origins[int(g.integers(0, len(origins)))], int(g.integers(1, 4))
        got = roi.track_origin(box, prev, h, w, H, W, hold)
        assert got == TR.track_origin(box, prev, h, w, H, W, hold), (box, prev, hold)
        assert 0 <= got[0] <= H - h and 0 <= got[1] <= W - w
        # an axis depends on its own coordinates alone
        other = boxes[int(g.integers(0, len(boxes) - 1))]
        assert roi.track_origin((box[0], other[1], box[2], other[3]), (prev[0], 0), h, w, H, W, hold)[0] == got[0] or roi.is_empty(box)
        n += 1
    for box in boxes:
        assert roi.track_origin(box, None, h, w, H, W, 1) == TR.track_origin(box, None, h, w, H, W, 1) == roi.window_origin(box, h, w, H, W)
    assert n > 20000


def test_track_origin_edge_cases():
    from otvm_amd import roi
    H, W, h, w = 12, 14, 5, 6
    both = lambda *a: (roi.track_origin(*a), TR.track_origin(*a))                      # noqa: E731

    def same(*a):
        got, want = both(*a)
        assert got == want, a
        return got
    # an empty box keeps the neighbour's origin on both axes; with no neighbour it is (0, 0)
    assert same((H, W, -1, -1), (3, 4), h, w, H, W, 2) == (3, 4)
    assert same((H, W, -1, -1), None, h, w, H, W, 2) == (0, 0)
    assert same((5, 5, 4, 9), (3, 4), h, w, H, W, 2) == (3, 4)                          # empty on one axis is empty
    # held: the box keeps `hold` pixels from both sides (window rows 3 .. 7, columns 4 .. 9)
    assert same((5, 6, 5, 7), (3, 4), h, w, H, W, 2) == (3, 4)
    # one pixel closer to the top: y recentres, (4 + 4 + 1) // 2 - 5 // 2 = 2, x holds
    assert same((4, 6, 4, 7), (3, 4), h, w, H, W, 2) == (2, 4)
    # x alone: columns 8 .. 9 reach the right side -> (8 + 9 + 1) // 2 - 3 = 6
    assert same((5, 8, 5, 9), (3, 4), h, w, H, W, 1) == (3, 6)
    # hold = 1: touching a side moves, one pixel off does not
    assert same((3, 6, 3, 6), (3, 4), h, w, H, W, 1) == (1, 4)
    assert same((4, 5, 6, 8), (3, 4), h, w, H, W, 1) == (3, 4)
    # a box larger than the window: centred on it, then clamped
    assert same((0, 0, 11, 13), (3, 4), h, w, H, W, 1) == (4, 4)
    assert same((1, 0, 11, 13), (0, 0), h, w, H, W, 1) == (4, 4)
    # a window flush against each frame side: that side always counts as held
    assert same((0, 6, 1, 7), (0, 4), h, w, H, W, 3) == (0, 4)                          # top
    assert same((10, 6, 11, 7), (H - h, 4), h, w, H, W, 3) == (H - h, 4)               # bottom
    assert same((5, 0, 5, 1), (3, 0), h, w, H, W, 2) == (3, 0)                          # left
    assert same((5, 12, 5, 13), (3, W - w), h, w, H, W, 2) == (3, W - w)               # right
    # ... but its other side does not
    assert same((0, 6, 4, 7), (0, 4), h, w, H, W, 1) == (0, 4)
    assert same((2, 6, 4, 7), (0, 4), h, w, H, W, 1) == (1, 4)
    # a window equal to the frame never moves
    for box in ((0, 0, 11, 13), (3, 3, 4, 4), (H, W, -1, -1)):
        assert same(box, (0, 0), H, W, H, W, 3) == (0, 0) and same(box, None, H, W, H, W, 3) == (0, 0)
    assert roi.hold_of(32) == 16 and roi.hold_of(16) == 8 and roi.hold_of(1) == 1 and roi.hold_of(0) == 1 == TR.hold_of(0)


def test_the_issue_clip_gives_the_simulated_windows():
    """The route test's clip (tests/test_gpu_roi_track.py), simulated on the host alone: a 96x96 window, hold 8, seven distinct
    origins from (0, 0) to (37, 84), no clipped frame; the faster clip outruns the held y axis and is first cut on frame 4 (its box
    is 53 pixels in a 96-pixel window: 21 to spare, 11 rows a frame, and a held axis lags two frames)."""
    from otvm_amd import roi
    from tests import mask_trimap_ref as MR
    from tests import roi_ref as R
    H, W, T = 160, 224, 8
    yy, xx = np.mgrid[0:H, 0:W]
    for (dy, dx), want_clipped in (((9, 14), []), ((11, 17), [4, 6])):
        ms = [np.floor(np.clip((20 - np.sqrt((yy - 40 - dy * t) ** 2 + (xx - 48 - dx * t) ** 2)) / 3.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)
              for t in range(T)]
        tri0 = MR.trimap_from_mask(ms[0], 6)
        labs = [MR.labels_from_mask(m, 6, band_label=1) for m in ms]
        size = roi.window_size([tuple(R.bbox(tri0)[4:])] + [tuple(R.bbox(l)[4:]) for l in labs[1:]], H, W, 16)
        assert size == (96, 96) and roi.hold_of(16) == 8
        wins, clipped = TR.clip_windows(size, H, W, 8, range(T), {0: tri0}, 0, [tri0] + labs[1:])
        assert clipped == want_clipped
        if not want_clipped:
            assert wins[0][:2] == (0, 0) and wins[T - 1][:2] == (37, 84) and len({wins[t][:2] for t in wins}) == 7


# ------------------------------------------------------------------ the binding
def test_binding_declares_the_tracking_entry_points():
    import __graft_entry__ as g
    from otvm_amd import lib as L
    h = ctypes.CDLL(g.build())
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    for sym in ("otvm_roi_track", "otvm_roi_crop_at", "otvm_roi_paste_at"):
        assert sym in L.EXPORTED and getattr(h, sym) is not None
    assert re.search(r"\bint otvm_roi_track\(const otvm_roi_track_params\* p, void\* stream\);", header)
    assert re.search(r"\bint otvm_roi_crop_at\(const otvm_roi_crop_params\* p, const int32_t\* origin, void\* stream\);", header)
    assert re.search(r"\bint otvm_roi_paste_at\(const otvm_roi_paste_params\* p, const int32_t\* origin, void\* stream\);", header)
    h.otvm_abi_version.restype = ctypes.c_int
    assert h.otvm_abi_version() == 21 == L.ABI_VERSION and "#define OTVM_ABI_VERSION 21 " in header
    body = header[header.index("typedef struct otvm_roi_track_params {"):header.index("} otvm_roi_track_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl.strip())
        names += [x.strip().lstrip("*") for x in decl.split(",") if x.strip()]
    assert names == [f for f, _ in L.RoiTrackParams._fields_]
    # the existing structs are taken as they are
    assert (ctypes.sizeof(L.RoiBboxParams), ctypes.sizeof(L.RoiCropParams), ctypes.sizeof(L.RoiPasteParams)) == (32, 72, 104)


def test_the_new_struct_has_the_size_gcc_gives_it():
    from otvm_amd import lib as L
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "otvm_hip.h"\n'
           'int main(void) { printf("%zu %zu %zu", sizeof(otvm_roi_track_params), offsetof(otvm_roi_track_params, out), '
           'offsetof(otvm_roi_track_params, hold)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    T = L.RoiTrackParams
    assert got == [ctypes.sizeof(T), T.out.offset, T.hold.offset] == [48, 16, 40]


def test_bad_arguments_of_the_tracking_entry_points_are_refused_before_any_launch():
    """The checks precede the launch, so they answer without a device: nonzero, and the message starts with the function's name."""
    import __graft_entry__ as g
    from otvm_amd import lib as L
    g.build()
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    at = ctypes.addressof(buf)

    def refused(rc, name):
        assert rc != 0
        assert lib.otvm_last_error().decode().startswith(name + ":"), lib.otvm_last_error()

    sizes = (dict(h=0), dict(w=0), dict(h=9), dict(w=13), dict(H=0), dict(W=0), dict(H=16384), dict(W=16384), dict(h=-1), dict(h=2 ** 31 - 1))
    for kw in sizes + (dict(box=None), dict(out=None), dict(hold=0), dict(hold=-3), dict(hold=16384), dict(prev=at + 2), dict(box=at + 1)):
        p = L.RoiTrackParams()
        p.box, p.prev, p.out, p.H, p.W, p.h, p.w, p.hold = at, at + 32, at + 64, 8, 12, 4, 4, 2
        for k, v in kw.items():
            setattr(p, k, v)
        refused(lib.otvm_roi_track(ctypes.byref(p), None), "otvm_roi_track")
    refused(lib.otvm_roi_track(None, None), "otvm_roi_track")
    for kw in sizes + (dict(frame_out=None), dict(frame=None), dict(origin=None), dict(origin=at + 2)):
        p = L.RoiCropParams()
        p.H, p.W, p.y0, p.x0, p.h, p.w, p.frame, p.frame_out = 8, 12, 1, 1, 4, 4, at, at
        origin = kw.pop("origin", at + 128) if "origin" in kw else at + 128
        for k, v in kw.items():
            setattr(p, k, v)
        refused(lib.otvm_roi_crop_at(ctypes.byref(p), origin, None), "otvm_roi_crop_at")
    refused(lib.otvm_roi_crop_at(None, at, None), "otvm_roi_crop_at")
    for kw in sizes + (dict(alpha=None), dict(win_alpha=None), dict(win_trimap=None), dict(fgr=at), dict(fgr=at, win_fgr=at),
                       dict(fgr=at, frame=at), dict(origin=None), dict(origin=at + 1)):
        p = L.RoiPasteParams()
        p.H, p.W, p.y0, p.x0, p.h, p.w, p.win_alpha, p.win_trimap, p.alpha = 8, 12, 1, 1, 4, 4, at, at, at
        origin = kw.pop("origin", at + 128) if "origin" in kw else at + 128
        for k, v in kw.items():
            setattr(p, k, v)
        refused(lib.otvm_roi_paste_at(ctypes.byref(p), origin, None), "otvm_roi_paste_at")
    refused(lib.otvm_roi_paste_at(None, at, None), "otvm_roi_paste_at")


# ------------------------------------------------------------------ refusals that need no device
class _NoDevice(torch.nn.Module):
    DILATION_KERNEL = 12

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0

    def forward(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the model was touched")


def test_track_refusals_come_before_the_model_is_touched():
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    model = _NoDevice()
    H, W, T = 40, 48, 3
    frames = [np.zeros((H, W, 3), np.uint8)] * T
    m = np.zeros((H, W), np.uint8)
    tri = np.zeros((3, H, W), np.float32)
    for roi in ("track", ("track", 32, 32)):
        for kw, word in ((dict(masks=[m] * T), "masks"),
                         (dict(trimap=tri, work_scale=2), "work_scale"),
                         (dict(alphas=[m] * T), "alphas"),
                         (dict(trimap=tri, backgrounds=frames), "backgrounds"),
                         (dict(trimap=tri, roi_margin=-1), "roi_margin"),
                         (dict(), "trimap flow")):
            with pytest.raises(ValueError, match=word):
                run_video_matte(model, frames, roi=roi, **kw)
        with pytest.raises(ValueError, match="float frames"):
            run_video_matte(model, [f.astype(np.float32) for f in frames], trimap=tri, roi=roi)
        with pytest.raises(ValueError, match="single-clip"):
            run_video_matte_batch(model, [frames], trimaps=[tri], roi=roi)
    # a size of the caller's: 1 <= h <= H and 1 <= w <= W, integers
    for bad, word in ((("track", 41, 32), "1 <= h <= 40"), (("track", 32, 49), "1 <= w <= 48"), (("track", 0, 32), "h, w >= 1"),
                      (("track", 32, -1), "h, w >= 1"), (("track", 32.5, 32), "h, w >= 1"), (("track", True, 32), "h, w >= 1")):
        with pytest.raises(ValueError, match=word):
            run_video_matte(model, frames, trimap=tri, roi=bad)
    # what is neither form is told what the forms are, 'auto' included
    for bad in ("tracking", "Track"):
        with pytest.raises(ValueError, match="'auto'"):
            run_video_matte(model, frames, trimap=tri, roi=bad)
    with pytest.raises(ValueError, match="four integers"):
        run_video_matte(model, frames, trimap=tri, roi=("track", 32))
    assert model.calls == 0


def test_eval_cli_parses_roi_track(tmp_path):
    from otvm_amd import eval_cli
    assert eval_cli.parse_roi_options("track", None) == ("track", 32)
    assert eval_cli.parse_roi_options("track,96,128", 16) == (("track", 96, 128), 16)
    data = str(tmp_path)
    for argv, word in ((["--roi", "track"], "--demo"), (["--demo", "--roi", "track", "--work-scale", "2"], "--work-scale"),
                       (["--demo", "--roi", "track", "--viz"], "--viz"), (["--demo", "--roi", "track", "--batch", "2"], "--batch"),
                       (["--demo", "--roi", "track,0,5"], "--roi"), (["--demo", "--roi", "track,5"], "--roi"),
                       (["--demo", "--roi", "track,a,b"], "--roi"), (["--demo", "--roi", "track", "--masks", "frame"], "--masks")):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(["--data", data, "--synthetic-weights"] + argv)
        assert word in str(e.value), (argv, str(e.value))
