"""GPU (-m gpu): region-of-interest matting -- otvm_trimap_bbox, otvm_roi_crop and otvm_roi_paste against their numpy restatement
(tests/roi_ref.py) bit for bit, determinism and refusals, and the routes through run_video_matte(roi=...) and eval_cli --roi
against the definition: the matte of the host-cropped clip, pasted back."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import fgr_ref
from tests import mask_trimap_ref as MR
from tests import roi_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(1, 1), (1, 37), (37, 1), (7, 300), (33, 70), (135, 241)]
JUNK = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from otvm_amd import lib as L
    return L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------ otvm_trimap_bbox
def _bbox_raw(lib, out, trimap=None, labels=None, H=None, W=None):
    from otvm_amd import lib as L
    p = L.RoiBboxParams()
    src = trimap if trimap is not None else labels
    p.trimap = None if trimap is None else trimap.data_ptr()
    p.labels = None if labels is None else labels.data_ptr()
    p.H, p.W = (src.shape[-2] if H is None else H), (src.shape[-1] if W is None else W)
    p.out = None if out is None else out.data_ptr()
    rc = lib.otvm_trimap_bbox(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc


def _class_maps(H, W, seed):
    """(name, class map [H,W] with 0 bg, 1 unknown, 2 fg) that put the boxes where indexing can go wrong."""
    g = np.random.default_rng(seed)
    out = [("all-bg", np.zeros((H, W), np.uint8)), ("all-unknown", np.ones((H, W), np.uint8)), ("all-fg", np.full((H, W), 2, np.uint8))]
    for name, (y, x) in (("tl", (0, 0)), ("tr", (0, W - 1)), ("bl", (H - 1, 0)), ("br", (H - 1, W - 1))):
        c = np.zeros((H, W), np.uint8)
        c[y, x] = 1
        c[H - 1 - y, W - 1 - x] = 2 if (H - 1 - y, W - 1 - x) != (y, x) else 1      # a foreground pixel in the opposite corner
        out.append(("corner-" + name, c))
    for name, sl in (("top", (slice(0, 1), slice(W // 3, W // 3 + 1))), ("bottom", (slice(H - 1, H), slice(W // 2, W // 2 + 1))),
                     ("left", (slice(H // 2, H // 2 + 1), slice(0, 1))), ("right", (slice(H // 3, H // 3 + 1), slice(W - 1, W)))):
        c = np.zeros((H, W), np.uint8)
        c[H // 2, W // 2] = 2
        c[sl] = 1
        out.append(("side-" + name, c))
    out.append(("random", g.choice(np.array([0, 1, 2], np.uint8), size=(H, W), p=(0.98, 0.01, 0.01))))
    return out


def _check_bbox_forms(lib, name, cls, H, W):
    onehot = np.stack([(cls == k) for k in range(3)]).astype(np.float32)
    lab = cls.copy()
    lab[(cls == 0) & (np.arange(H * W).reshape(H, W) % 5 == 0)] = 255              # unlabelled pixels count as nothing
    for form, src in (("trimap", onehot), ("labels", lab)):
        want = R.bbox(src)
        rows = torch.full((3, 8), JUNK, dtype=torch.int32, device=DEV)               # out pre-filled with junk; slot 1 of a [T,8] buffer
        d = dev(src)
        assert _bbox_raw(lib, rows[1], **{form: d}) == 0, (name, form)
        got = rows.cpu().numpy()
        assert np.array_equal(got[1], want), (name, form, got[1], want)
        assert (got[0] == JUNK).all() and (got[2] == JUNK).all(), (name, form)       # the neighbours are not disturbed
        again = torch.full((8,), -JUNK, dtype=torch.int32, device=DEV)
        assert _bbox_raw(lib, again, **{form: d}) == 0
        assert np.array_equal(again.cpu().numpy(), got[1]), (name, form)             # two calls, equal bits


@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_bbox_equals_the_restatement(lib, H, W):
    for name, cls in _class_maps(H, W, 7 * H + W):
        _check_bbox_forms(lib, name, cls, H, W)
    # probabilities on a coarse grid: the ties t1 == t2 and t0 == max(t1, t2)
    g = np.random.default_rng(H + 3 * W)
    prob = (g.integers(0, 4, size=(3, H, W)) / 4.0).astype(np.float32)
    prob[0] = np.maximum(prob[0], (g.random((H, W)) < 0.9).astype(np.float32))       # mostly background: the boxes vary
    out = torch.full((8,), JUNK, dtype=torch.int32, device=DEV)
    assert _bbox_raw(lib, out, trimap=dev(prob)) == 0
    assert np.array_equal(out.cpu().numpy(), R.bbox(prob))


def test_bbox_python_wrapper_and_read_back(lib):
    from otvm_amd import roi
    H, W, T = 33, 70, 4
    g = np.random.default_rng(5)
    rows = torch.full((T, 8), JUNK, dtype=torch.int32, device=DEV)
    maps = [g.choice(np.array([0, 1, 2, 255], np.uint8), size=(H, W), p=(0.9, 0.03, 0.03, 0.04)) for _ in range(T)]
    maps[2] = np.zeros((H, W), np.uint8)
    for t in range(T):
        roi.trimap_bbox(dev(maps[t]), rows[t])
    unknown, nonbg = roi.boxes_of(rows)                                              # ONE copy for the clip
    for t in range(T):
        want = R.bbox(maps[t]).tolist()
        assert unknown[t] == tuple(want[:4]) and nonbg[t] == tuple(want[4:]), t
    assert unknown[2] == (H, W, -1, -1) and roi.is_empty(unknown[2])
    onehot = np.stack([(maps[0] == k) for k in range(3)]).astype(np.float32)
    assert roi.trimap_bbox(dev(onehot)).cpu().tolist() == R.bbox(onehot).tolist()
    with pytest.raises(ValueError, match="float32 trimap"):
        roi.trimap_bbox(dev(onehot).double())


# ------------------------------------------------------------------------------------------------ otvm_roi_crop / otvm_roi_paste
def _windows(H, W):
    h, w = max(1, H // 2), max(1, (W // 2) | 1 if W > 2 else 1)
    wins = [(0, 0, h, w), (0, W - w, h, w), (H - h, 0, h, w), (H - h, W - w, h, w), (0, 0, H, W)]
    if H >= 33 and W >= 70:
        wins += [(1, 37, 32, 32), (H - 32, 3, 32, 64)]                               # aligned window sizes at odd origins
    if W >= 5:
        wins.append((H // 3, 1 if W % 2 else 3, max(1, H // 3), W - 4))              # an odd x0
    return sorted(set(wins))


def _frame_inputs(H, W, seed):
    g = np.random.default_rng(seed)
    frame = g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    cls = g.choice(3, size=(H, W))
    tri = np.stack([(cls == k) for k in range(3)]).astype(np.float32)
    lab = g.choice(np.array([0, 1, 2, 255], np.uint8), size=(H, W))
    return frame, tri, lab


def _crop_raw(lib, win, H, W, frame=None, trimap=None, labels=None, outs=None):
    """One otvm_roi_crop call on outputs pre-filled with junk -> (rc, frame, trimap, labels)"""
    from otvm_amd import lib as L
    y0, x0, h, w = win
    p = L.RoiCropParams()
    p.H, p.W, p.y0, p.x0, p.h, p.w = H, W, y0, x0, h, w
    hh, ww = max(h, 1), max(w, 1)
    if outs is None:
        outs = (None if frame is None else torch.full((hh, ww, 3), 77, dtype=torch.uint8, device=DEV),
                None if trimap is None else torch.full((3, hh, ww), -7.0, dtype=torch.float32, device=DEV),
                None if labels is None else torch.full((hh, ww), 77, dtype=torch.uint8, device=DEV))
    for name, src, dst in zip(("frame", "trimap", "labels"), (frame, trimap, labels), outs):
        setattr(p, name, None if src is None else src.data_ptr())
        setattr(p, name + "_out", None if dst is None else dst.data_ptr())
    rc = lib.otvm_roi_crop(C.byref(p), stream())
    torch.cuda.synchronize()
    return (rc,) + tuple(outs)


def _paste_raw(lib, win, H, W, alpha, tri, fgr=None, frame=None, rgb=0, outside=None, want=("alpha", "alpha_u8", "trimap", "fgr")):
    """One otvm_roi_paste call on outputs pre-filled with junk -> (rc, {name: tensor})"""
    from otvm_amd import lib as L
    y0, x0, h, w = win
    p = L.RoiPasteParams()
    p.H, p.W, p.y0, p.x0, p.h, p.w, p.u8_rgb = H, W, y0, x0, h, w, rgb
    p.win_alpha, p.win_trimap = alpha.data_ptr(), tri.data_ptr()
    p.win_fgr = None if fgr is None else fgr.data_ptr()
    p.frame = None if frame is None else frame.data_ptr()
    p.outside = None if outside is None else outside.data_ptr()
    HH, WW = max(H, 1), max(W, 1)
    outs = {}
    for name, shape, dt, fill in (("alpha", (HH, WW), torch.float32, -7.0), ("alpha_u8", (HH, WW), torch.uint8, 77),
                                  ("trimap", (3, HH, WW), torch.float32, -7.0), ("fgr", (3, HH, WW), torch.float32, -7.0)):
        if name in want:
            outs[name] = torch.full(shape, fill, dtype=dt, device=DEV)
            setattr(p, name, outs[name].data_ptr())
    rc = lib.otvm_roi_paste(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc, outs


def _window_results(h, w, seed, nan=True):
    g = np.random.default_rng(seed)
    alpha = (g.random((h, w)) * 1.2 - 0.1).astype(np.float32)                        # a little outside [0,1]: the byte clamps
    if nan:
        alpha[h // 2, w // 2] = np.nan                                               # a non-finite alpha gives byte 0
        alpha[0, 0] = np.inf if h * w > 1 else alpha[0, 0]
    tri = g.random((3, h, w)).astype(np.float32)
    fgr = (g.random((3, h, w)) * 1.1).astype(np.float32)
    return alpha, tri, fgr


def _check_paste(lib, win, H, W, frame, outside_np, rgb, with_fgr, want, seed):
    alpha, tri, fgr = _window_results(win[2], win[3], seed)
    w_alpha, w_u8, w_tri, w_fgr = R.paste(win, H, W, alpha, tri, fgr if with_fgr else None, frame, bool(rgb), outside_np)
    rc, outs = _paste_raw(lib, win, H, W, dev(alpha), dev(tri), dev(fgr) if with_fgr else None, dev(frame) if with_fgr else None, rgb,
                          None if outside_np is None else dev(outside_np), want)
    what = (win, H, W, rgb, with_fgr, outside_np is not None, want)
    assert rc == 0, what
    for name, ref in (("alpha", w_alpha), ("alpha_u8", w_u8), ("trimap", w_tri), ("fgr", w_fgr)):
        if name in want:
            assert np.array_equal(bits(outs[name]), bits(ref)), what + (name,)       # every element, junk included, is written
    if "alpha_u8" in want:
        y0, x0, h, w = win
        assert outs["alpha_u8"][y0 + h // 2, x0 + w // 2].item() == 0                # the NaN


@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_crop_and_paste_equal_the_restatement(lib, H, W):
    frame, tri, lab = _frame_inputs(H, W, 11 * H + W)
    g = np.random.default_rng(W)
    ocls = g.choice(3, size=(H, W))
    outside = np.stack([(ocls == k) for k in range(3)]).astype(np.float32)
    fd, td, ld = dev(frame), dev(tri), dev(lab)
    for j, win in enumerate(_windows(H, W)):
        wf, wt, wl = R.crop(win, frame, tri, lab)
        rc, gf, gt, gl = _crop_raw(lib, win, H, W, fd, td, ld)
        assert rc == 0 and np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(bits(gt), bits(wt)) and np.array_equal(gl.cpu().numpy(), wl), win
        # each destination alone
        assert np.array_equal(_crop_raw(lib, win, H, W, frame=fd)[1].cpu().numpy(), wf), win
        assert np.array_equal(bits(_crop_raw(lib, win, H, W, trimap=td)[2]), bits(wt)), win
        assert np.array_equal(_crop_raw(lib, win, H, W, labels=ld)[3].cpu().numpy(), wl), win
        for rgb in (0, 1):
            for out_np in (None, outside):
                _check_paste(lib, win, H, W, frame, out_np, rgb, True, ("alpha", "alpha_u8", "trimap", "fgr"), 100 * j + rgb)
        _check_paste(lib, win, H, W, frame, outside, 0, False, ("alpha", "alpha_u8", "trimap"), j)          # without F
        for absent in ("alpha", "alpha_u8", "trimap", "fgr"):                                               # each output absent
            _check_paste(lib, win, H, W, frame, None, 1, True, tuple(n for n in ("alpha", "alpha_u8", "trimap", "fgr") if n != absent), j)


def test_kernels_equal_the_restatement_at_1080p_every_element(lib):
    H, W = 1080, 1920
    frame, tri, lab = _frame_inputs(H, W, 3)
    cls = np.zeros((H, W), np.uint8)
    cls[301:777, 403:1202] = 2
    cls[290:301, 403:1202] = 1
    cls[777:790, 380:1210] = 1
    onehot = np.stack([(cls == k) for k in range(3)]).astype(np.float32)
    for form, src in (("trimap", onehot), ("labels", cls), ("trimap", tri), ("labels", lab)):
        out = torch.full((8,), JUNK, dtype=torch.int32, device=DEV)
        assert _bbox_raw(lib, out, **{form: dev(src)}) == 0
        assert np.array_equal(out.cpu().numpy(), R.bbox(src)), form
    assert R.bbox(onehot).tolist() == [290, 380, 789, 1209, 290, 380, 789, 1209]
    win = (283, 379, 512, 640)
    wf, wt, wl = R.crop(win, frame, tri, lab)
    rc, gf, gt, gl = _crop_raw(lib, win, H, W, dev(frame), dev(tri), dev(lab))
    assert rc == 0 and np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(bits(gt), bits(wt)) and np.array_equal(gl.cpu().numpy(), wl)
    for rgb, out_np in ((0, None), (1, onehot)):
        _check_paste(lib, win, H, W, frame, out_np, rgb, True, ("alpha", "alpha_u8", "trimap", "fgr"), rgb)


def test_python_wrappers_crop_and_paste(lib):
    from otvm_amd import roi
    H, W, win = 33, 71, (1, 37, 32, 32)
    frame, tri, lab = _frame_inputs(H, W, 9)
    gf, gt, gl = roi.crop(win, frame=dev(frame), trimap=dev(tri), labels=dev(lab))
    wf, wt, wl = R.crop(win, frame, tri, lab)
    assert np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(bits(gt), bits(wt)) and np.array_equal(gl.cpu().numpy(), wl)
    assert roi.crop(win, labels=dev(lab))[:2] == (None, None)
    alpha, wtri, fgr = _window_results(32, 32, 1)
    got = roi.paste(win, H, W, dev(alpha), dev(wtri), dev(fgr), dev(frame), rgb=True, outside=dev(tri))
    for g_, w_ in zip(got, R.paste(win, H, W, alpha, wtri, fgr, frame, True, tri)):
        assert np.array_equal(bits(g_), bits(w_))
    got = roi.paste(win, H, W, dev(alpha), dev(wtri), want=("alpha_u8",))
    assert got[0] is None and got[2] is None and got[3] is None
    assert np.array_equal(got[1].cpu().numpy(), R.paste(win, H, W, alpha, wtri)[1])
    with pytest.raises(ValueError, match="leaves the 33x71 frame"):
        roi.crop((2, 37, 32, 32), frame=dev(frame))
    with pytest.raises(ValueError, match="leaves"):
        roi.paste((1, 40, 32, 32), H, W, dev(alpha), dev(wtri))


def test_bad_arguments_return_nonzero_and_leave_the_outputs_untouched(lib):
    H, W = 33, 70
    frame, tri, lab = _frame_inputs(H, W, 2)
    fd, td, ld = dev(frame), dev(tri), dev(lab)

    def said(name):
        assert lib.otvm_last_error().decode().startswith(name + ":"), lib.otvm_last_error()
    out = torch.full((8,), JUNK, dtype=torch.int32, device=DEV)
    for kw in (dict(trimap=td, labels=ld), dict(H=H, W=W), dict(labels=ld, H=0), dict(labels=ld, W=0), dict(labels=ld, H=16384),
               dict(trimap=td, W=16384)):
        kw = {"H": H, "W": W, **kw}
        assert _bbox_raw(lib, out, **kw) != 0, kw
        said("otvm_trimap_bbox")
    assert (out.cpu().numpy() == JUNK).all()
    alpha, wtri, fgr = (dev(x) for x in _window_results(8, 8, 0))
    for win, hw in (((0, 0, 0, 8), (H, W)), ((0, 0, 8, 0), (H, W)), ((26, 0, 8, 8), (H, W)), ((0, 63, 8, 8), (H, W)), ((-1, 0, 8, 8), (H, W)),
                    ((0, -1, 8, 8), (H, W)), ((0, 0, 8, 8), (0, W)), ((0, 0, 8, 8), (H, 0)), ((0, 0, 8, 8), (16384, W)),
                    ((0, 0, 8, 8), (H, 16384))):
        outs = (torch.full((8, 8, 3), 77, dtype=torch.uint8, device=DEV), torch.full((3, 8, 8), -7.0, device=DEV),
                torch.full((8, 8), 77, dtype=torch.uint8, device=DEV))
        rc = _crop_raw(lib, win, hw[0], hw[1], fd, td, ld, outs=outs)[0]
        assert rc != 0, (win, hw)
        said("otvm_roi_crop")
        assert (outs[0] == 77).all() and (outs[1] == -7.0).all() and (outs[2] == 77).all(), (win, hw)
        if hw == (H, W):                                                             # (the junk-filled outputs are H x W)
            rc, po = _paste_raw(lib, win, H, W, alpha, wtri, fgr, fd)
            assert rc != 0, win
            said("otvm_roi_paste")
            assert (po["alpha"] == -7.0).all() and (po["alpha_u8"] == 77).all() and (po["trimap"] == -7.0).all() and (po["fgr"] == -7.0).all()
    rc, po = _paste_raw(lib, (0, 0, 8, 8), H, W, alpha, wtri, None, fd)              # fgr without the window's F
    assert rc != 0 and (po["fgr"] == -7.0).all() and (po["alpha"] == -7.0).all()
    rc, po = _paste_raw(lib, (0, 0, 8, 8), H, W, alpha, wtri, fgr, fd, want=())       # no output
    assert rc != 0
    assert _crop_raw(lib, (0, 0, 8, 8), H, W, outs=(None, None, None))[0] != 0        # no destination


# ------------------------------------------------------------------------------------------------ routes
H_, W_, T_, BAND = 160, 224, 5, 6


def _clip():
    """Five frames of the synthetic clip and a soft mask per frame: a disc of radius 20 that moves (3, 5) pixels a frame."""
    from otvm_amd.synth_data import synthetic_clip
    frames, _ = synthetic_clip(H_, W_, T_, seed=29)
    yy, xx = np.mgrid[0:H_, 0:W_]
    ms = []
    for t in range(T_):
        r = np.sqrt((yy - 60 - 3 * t) ** 2 + (xx - 70 - 5 * t) ** 2)
        ms.append(np.floor(np.clip((20 - r) / 3.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8))
    return [np.ascontiguousarray(f) for f in frames], ms, [MR.trimap_from_mask(m, BAND) for m in ms]


@pytest.fixture(scope="module")
def route(lib, synth_sd, tmp_path_factory):
    """One model for all route tests, with the kernel configurations fixed and shared through a file (eval_cli's own model
    launches the same ones)."""
    from otvm_amd import engine
    from tests.test_gpu_frame import _fresh_model
    old, old_auto = os.environ.get("OTVM_TUNE_FILE"), engine.AUTOTUNE
    os.environ["OTVM_TUNE_FILE"] = os.path.join(str(tmp_path_factory.mktemp("tune")), "tune.json")
    engine.AUTOTUNE = False
    try:
        yield (_fresh_model(synth_sd, 12, "f16x3"),) + _clip()
    finally:
        engine.AUTOTUNE = old_auto
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a.contiguous()), bits(b.contiguous()))


def _inside(x, win):
    y0, x0, h, w = win
    return x[..., y0:y0 + h, x0:x0 + w]


def _outside_mask(win):
    m = np.ones((H_, W_), bool)
    m[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = False
    return torch.from_numpy(m)


def _crop_clip(frames, win):
    y0, x0, h, w = win
    return [np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]) for f in frames]


def _masks(ms, **kw):
    from otvm_amd.masks import Mask
    return [Mask(m, band=BAND, **kw) for m in ms]


KW = dict(skip=2, max_num=3)


def test_masks_route_tracks_the_unknown_band(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris = route
    got = run_video_matte(m, frames, masks=_masks(ms), roi="auto", roi_margin=0, **KW)
    wins = R.tracking_windows([tuple(R.bbox(t)[:4]) for t in tris], H_, W_, 0)
    assert got["roi"] == wins and got["roi_size"] == (64, 64) and got["roi_clipped"] == []
    assert len({w[:2] for w in wins}) > 1                                            # the window follows the subject
    assert got["bank_frames"] == [[]] * T_
    assert tuple(got["alpha"].shape) == (T_, H_, W_) and tuple(got["trimap"].shape) == (T_, 3, H_, W_)
    for t, win in enumerate(wins):
        one = run_video_matte(m, _crop_clip(frames[t:t + 1], win), trimap=R.crop(win, trimap=tris[t])[1], **KW)
        for k in ("alpha", "alpha_u8", "trimap"):
            assert _eq(_inside(got[k][t], win), one[k][0]), (k, t)
        out = _outside_mask(win)
        fg = torch.from_numpy(tris[t][2])
        assert torch.equal(got["alpha"][t][out], fg[out]) and set(got["alpha"][t][out].unique().tolist()) <= {0.0, 1.0}, t
        assert torch.equal(got["alpha_u8"][t][out], (fg[out] * 255).to(torch.uint8)), t
        assert torch.equal(got["trimap"][t][:, out], torch.from_numpy(tris[t])[:, out]), t
    # a window of the caller's serves every frame
    win = (32, 40, 96, 128)
    user = run_video_matte(m, frames, masks=_masks(ms), roi=win, **KW)
    assert user["roi"] == [win] * T_ and user["roi_size"] == (96, 128)
    one = run_video_matte(m, _crop_clip(frames[3:4], win), trimap=R.crop(win, trimap=tris[3])[1], **KW)
    assert _eq(_inside(user["alpha"][3], win), one["alpha"][0]) and _eq(_inside(user["trimap"][3], win), one["trimap"][0])


def test_trimap_route_in_a_static_window(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris = route
    win = (30, 40, 64, 96)
    got = run_video_matte(m, frames, trimap=tris[0], roi=win, **KW)
    want = run_video_matte(m, _crop_clip(frames, win), trimap=R.crop(win, trimap=tris[0])[1], **KW)
    for k in ("alpha", "alpha_u8", "trimap"):
        assert _eq(_inside(got[k], win), want[k]), k
    assert got["bank_frames"] == want["bank_frames"] and got["roi"] == [win] * T_ and got["roi_size"] == (64, 96)
    out = _outside_mask(win)
    assert (got["alpha"][:, out] == 0).all() and (got["alpha_u8"][:, out] == 0).all()
    assert (got["trimap"][:, 0][:, out] == 1).all() and (got["trimap"][:, 1:][:, :, out] == 0).all()
    auto = run_video_matte(m, frames[:2], trimap=tris[0], roi="auto", **KW)
    predicted = R.static_window([tuple(R.bbox(tris[0])[4:])], H_, W_, 32)
    assert auto["roi"] == [predicted] * 2 and auto["roi_size"] == predicted[2:]
    auto8 = run_video_matte(m, frames[:1], mask=_masks(ms)[0], roi="auto", roi_margin=8, **KW)
    assert auto8["roi"] == [R.static_window([tuple(R.bbox(tris[0])[4:])], H_, W_, 8)]


def test_keyframes_with_a_backward_sweep(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris = route
    lab = MR.labels_from_mask(ms[4], BAND, band_label=255)
    win = R.static_window([tuple(R.bbox(tris[2])[4:]), tuple(R.bbox(lab)[4:])], H_, W_, 8)
    got = run_video_matte(m, frames, keyframes={2: tris[2], 4: _masks(ms, role="labels")[4]}, roi="auto", roi_margin=8, **KW)
    want = run_video_matte(m, _crop_clip(frames, win), keyframes={2: R.crop(win, trimap=tris[2])[1], 4: R.crop(win, labels=lab)[2]}, **KW)
    assert got["roi"] == [win] * T_
    for k in ("alpha", "alpha_u8", "trimap"):
        assert _eq(_inside(got[k], win), want[k]), k
    assert got["schedule"] == want["schedule"] and got["schedule"][0][0] == 2 and got["schedule"][-1][0] == 0
    assert got["bank_frames"] == want["bank_frames"] and got["anchor_frames"] == want["anchor_frames"]


def test_foreground_bytes_are_made_from_the_pasted_planes(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris = route
    eng, seen = m.module, {}

    def keep(i, alpha, u8, out):
        seen[i] = (out[3][0, 0, 0].cpu().numpy(), out[1][0, 0].cpu().numpy(), eng._engine.last_fgr.cpu().numpy())
    colour = (10, 200, 30)
    got = run_video_matte(m, frames, masks=_masks(ms), roi="auto", roi_margin=0, foreground=True, new_background=colour, on_frame=keep, **KW)
    assert torch.equal(got["fgr_u8"][..., 3], got["alpha_u8"]) and m.module.foreground is False
    for t, win in enumerate(got["roi"]):
        a_w, t_w, f_w = seen[t]
        assert a_w.shape == (64, 64) and f_w.shape == (3, 64, 64)                    # on_frame's `out` is the network's, at the window's size
        alpha, u8, tri, F = R.paste(win, H_, W_, a_w, t_w, f_w, frames[t], False, tris[t])
        _, rgba, comp = fgr_ref.fgr_outputs(alpha, F, colour, u8_rgb=False)
        assert np.array_equal(got["fgr_u8"][t].numpy(), rgba) and np.array_equal(got["comp_u8"][t].numpy(), comp), t
        assert np.array_equal(got["alpha_u8"][t].numpy(), u8) and np.array_equal(bits(got["alpha"][t]), bits(alpha)), t
        out = _outside_mask(win).numpy()
        assert np.array_equal(got["fgr_u8"][t].numpy()[..., :3][out], frames[t][out]), t                    # the frame's own bytes
    handed = []
    res = run_video_matte(m, frames[:2], masks=_masks(ms)[:2], roi="auto", roi_margin=0, foreground=True, new_background=colour,
                          on_foreground=lambda i, rgba, comp: handed.append((i, rgba.cpu(), comp.cpu())), **KW)
    assert "fgr_u8" not in res and [h[0] for h in handed] == [0, 1]
    assert torch.equal(handed[1][1], got["fgr_u8"][1]) and torch.equal(handed[1][2], got["comp_u8"][1])


def test_stabiliser_runs_behind_the_paste(route):
    from otvm_amd.temporal import TemporalStabiliser
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris = route
    got = run_video_matte(m, frames, masks=_masks(ms), roi="auto", roi_margin=0, stabilise=True, foreground=True, **KW)
    plain = run_video_matte(m, frames, masks=_masks(ms), roi="auto", roi_margin=0, **KW)
    assert _eq(got["alpha_raw"], plain["alpha"]) and _eq(got["trimap"], plain["trimap"])
    st = TemporalStabiliser(DEV, H_, W_)
    outs = [st.step(dev(frames[t]), got["alpha_raw"][t].to(DEV), trimap=got["trimap"][t].to(DEV), tri_scale=1, rgb=False) for t in range(T_)]
    assert _eq(got["alpha"], torch.stack([o[0] for o in outs]).cpu()) and _eq(got["alpha_u8"], torch.stack([o[1] for o in outs]).cpu())
    assert not torch.equal(got["alpha"], got["alpha_raw"])                           # the filter acts on this clip
    assert torch.equal(got["fgr_u8"][..., 3], got["alpha_u8"])


def _clipped_by_definition(trimaps, wins):
    """The frames whose non-background box (restated) reaches a side of their window that is not a side of the frame."""
    out = []
    for t, (win, tri) in enumerate(zip(wins, trimaps)):
        y0, x0, h, w = win
        b = R.bbox(_inside(tri, win).numpy() if torch.is_tensor(tri) else tri)[4:]
        if b[2] >= b[0] and ((b[0] == 0 and y0 > 0) or (b[1] == 0 and x0 > 0) or (b[2] == h - 1 and y0 + h < H_) or (b[3] == w - 1 and x0 + w < W_)):
            out.append(t)
    return out


def test_roi_clipped_lists_the_frames_that_reach_the_window(route):
    from otvm_amd.video import _RegionOfInterest, run_video_matte
    m, frames, ms, tris = route
    # the stage alone, on hand-made outputs (synthetic weights propagate no subject): the disc's classes fill rows 34 ... 86 on
    # frame 0 and move 3 rows down a frame; the window's last row is 95, which they reach on frames 3 and 4.  Its columns they
    # never reach.
    win = (32, 40, 64, 96)

    class Plan:
        roi = (win, 32)
    region = _RegionOfInterest(Plan(), False, False, None)
    region.place_static({0: tuple(R.bbox(tris[0])[4:])}, H_, W_, T_)
    pasted = []
    for t in range(T_):
        region.full = dev(frames[t])
        w_tri = dev(R.crop(win, trimap=tris[t])[1])
        alpha, u8, tri = region.finish(t, (None, w_tri[None, None], None, w_tri[1][None, None, None].contiguous()), None, torch.device(DEV))
        pasted.append(tri.cpu())
        assert torch.equal(_inside(tri.cpu(), win), w_tri.cpu()) and torch.equal(_inside(alpha.cpu(), win), w_tri[1].cpu()), t
    res = region.result()
    assert res["roi_clipped"] == [3, 4] == _clipped_by_definition(pasted, [win] * T_)
    assert res["roi"] == [win] * T_ and res["roi_size"] == (64, 96)
    # the same window pushed against the frame's bottom: the side the disc reaches is the frame's own
    low = (H_ - 64, 40, 64, 96)
    region = _RegionOfInterest(type("Plan", (), {"roi": (low, 32)})(), False, False, None)
    region.place_static({}, H_, W_, 2)
    for t in range(2):
        region.full = dev(frames[t])
        tri = np.zeros((3, 64, 96), np.float32)
        tri[0] = 1
        tri[:, 40:64, 20:50] = np.array([0, 0, 1], np.float32)[:, None, None]           # down to the window's last row
        region.finish(t, (None, dev(tri)[None, None], None, dev(tri[2])[None, None, None]), None, torch.device(DEV))
    assert region.result()["roi_clipped"] == []
    # through the network: whatever it propagates, the list is the definition applied to the trimaps it returned
    got = run_video_matte(m, frames, trimap=tris[0], roi=win, **KW)
    assert got["roi_clipped"] == _clipped_by_definition(list(got["trimap"]), got["roi"])
    full = np.ascontiguousarray(np.stack([np.zeros((H_, W_)), np.ones((H_, W_)), np.zeros((H_, W_))]).astype(np.float32))
    whole = run_video_matte(m, frames[:2], trimap=full, roi=(0, 0, H_, W_), **KW)
    assert whole["roi_clipped"] == [] and whole["roi_size"] == (H_, W_) and whole["roi"] == [(0, 0, H_, W_)] * 2


def test_refusals_come_before_any_frame_and_leave_the_model_as_it_was(route):
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    m, frames, ms, tris = route
    before = run_video_matte(m, frames[:2], trimap=tris[0], **KW)
    calls = []
    handle = m.module.register_forward_pre_hook(lambda mod, args: calls.append(1))
    try:
        for kw, word in ((dict(trimap=tris[0], roi="auto", work_scale=2), "work_scale"),
                         (dict(alphas=[x.astype(np.float32) / 255 for x in ms], roi="auto"), "alphas"),
                         (dict(trimap=tris[0], backgrounds=list(frames), roi="auto"), "backgrounds"),
                         (dict(trimap=tris[0], roi="box"), "'auto'"), (dict(trimap=tris[0], roi=(0, 0, 64)), "four integers"),
                         (dict(trimap=tris[0], roi=(120, 0, 64, 64)), "leaves the 160x224 frame"),
                         (dict(trimap=tris[0], roi="auto", roi_margin=-2), "roi_margin"),
                         # a window of the caller's that does not hold a source's box / the unknown band of a later frame
                         (dict(trimap=tris[0], roi=(40, 40, 64, 64)), "frame 0"),
                         (dict(keyframes={0: tris[0], 4: tris[4]}, roi=(30, 40, 64, 96)), "frame 4"),
                         (dict(masks=_masks(ms), roi=(30, 40, 64, 96)), "unknown band of frame")):
            with pytest.raises(ValueError, match=word):
                run_video_matte(m, frames, **KW, **kw)
        with pytest.raises(ValueError, match="float frames"):
            run_video_matte(m, [f.astype(np.float32) for f in frames], trimap=tris[0], roi="auto")
        with pytest.raises(ValueError, match="single-clip"):
            run_video_matte_batch(m, [frames], trimaps=[tris[0]], roi="auto")
    finally:
        handle.remove()
    assert calls == []
    after = run_video_matte(m, frames[:2], trimap=tris[0], **KW)
    for k in ("alpha", "alpha_u8", "trimap"):
        assert _eq(before[k], after[k]), k
    assert before["bank_frames"] == after["bank_frames"] and sorted(after) == ["alpha", "alpha_u8", "bank_frames", "trimap"]


# ------------------------------------------------------------------------------------------------ eval_cli
def test_eval_cli_roi(tmp_path, route):
    import json
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.video import run_video_matte
    m, frames_bgr, ms, tris = route
    demo = os.path.join(str(tmp_path), "demo")
    for sub in ("frames", "mask"):
        os.makedirs(os.path.join(demo, "clip", sub))
    for t in range(T_):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
        Image.fromarray(ms[t]).save(os.path.join(demo, "clip", "mask", "%04d.png" % t))
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "2", "--mask-band", str(BAND)]
    out, sj = os.path.join(str(tmp_path), "out"), os.path.join(str(tmp_path), "s.json")
    res = eval_cli.main(common + ["--out", out, "--masks", "frame", "--roi", "auto", "--roi-margin", "0", "--fgr", "--summary-json", sj])
    assert res["frames"] == T_
    s = json.load(open(sj))
    assert s["roi"] == "auto" and s["roi_margin"] == 0 and s["roi_size"] == {"clip": [64, 64]} and s["roi_clipped"] == {"clip": []}
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames_bgr]
    ref = run_video_matte(m, rgb, masks=_masks(ms), roi="auto", roi_margin=0, skip=2, max_num=5, frames_are_rgb=True, foreground=True)
    for t in range(T_):
        a = np.asarray(Image.open(os.path.join(out, "alpha", "test", "s4_OTVM", "pred", "clip", "%04d.png" % t)))
        f = np.asarray(Image.open(os.path.join(out, "fgr", "clip", "%04d.png" % t)))
        assert np.array_equal(a, ref["alpha_u8"][t].numpy()), t
        assert np.array_equal(f, ref["fgr_u8"][t].numpy()), t                        # RGB frames: the PNG's order
    with pytest.raises(SystemExit, match="--work-scale"):
        eval_cli.main(common + ["--out", out, "--masks", "frame", "--roi", "auto", "--work-scale", "2"])
