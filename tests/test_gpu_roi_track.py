"""GPU (-m gpu): the tracking window of region-of-interest matting -- otvm_roi_track against its restatement
(tests/roi_track_ref.py) bit for bit, otvm_roi_crop_at / otvm_roi_paste_at against the host-origin kernels and the restatement,
and run_video_matte(roi="track") / eval_cli --roi track against the definition: the matte of the clip whose frame t is cropped on
the host at window t, pasted back."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import fgr_ref
from tests import mask_trimap_ref as MR
from tests import roi_ref as R
from tests import roi_track_ref as TR
from tests.test_gpu_roi import (SIZES, _crop_raw, _frame_inputs, _paste_raw, _window_results, _windows, bits, dev, stream)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from otvm_amd import lib as L
    return L.load()


# ------------------------------------------------------------------------------------------------ otvm_roi_track
def _track_cases(H, W):
    """(box row of eight words, previous origin or None, (h, w), hold): boxes at every corner and side of the window (of the frame
    without a previous origin), the empty box, a box larger than the window, for windows in a corner, in the middle and the
    frame itself."""
    cases = []
    for h, w in sorted({(max(1, H // 2), max(1, (W // 2) | 1 if W > 2 else 1)), (H, W), (min(H, 32), min(W, 32))}):
        origins = sorted({(0, 0), (H - h, W - w), ((H - h) // 2, (W - w) // 3), (0, W - w), (H - h, 0)})
        for hold in (1, 4):
            for prev in origins + [None]:
                sh, sw = (h, w) if prev is not None else (H, W)              # the space the box lives in
                ys = sorted({0, sh - 1, sh // 2, min(hold, sh - 1), max(sh - 1 - hold, 0)})
                xs = sorted({0, sw - 1, sw // 2, min(hold, sw - 1), max(sw - 1 - hold, 0)})
                boxes = [(y, x, y, x) for y in ys for x in xs]               # single pixels: corners, sides, at `hold` from them
                boxes += [(0, 0, sh - 1, sw - 1), (sh // 3, sw // 3, sh // 2, sw // 2), (sh, sw, -1, -1)]
                boxes += [(ys[1] if len(ys) > 1 else 0, 0, sh - 1, sw // 2), (0, xs[1] if len(xs) > 1 else 0, sh // 2, sw - 1)]
                if prev is None:
                    boxes += [(0, 0, min(H - 1, h), min(W - 1, w)), (H - 1 - min(H - 1, h), W - 1 - min(W - 1, w), H - 1, W - 1)]
                for b in boxes:
                    cases.append(((7, 7, 3, 3) + b, prev, (h, w), hold))      # (the unknown box, words 0 .. 3, is not looked at)
    return cases


@pytest.mark.parametrize("H,W", [(1, 1), (1, 37), (37, 1), (33, 70), (135, 241)], ids=lambda v: str(v))
def test_track_equals_the_restatement(lib, H, W):
    from otvm_amd import roi
    cases = _track_cases(H, W)
    n = len(cases)
    rows = dev(np.array([c[0] for c in cases], np.int32))
    prevs = dev(np.array([c[1] or (0, 0) for c in cases], np.int32))
    logs = [torch.full((2 * n + 1, 2), JUNK, dtype=torch.int32, device=DEV), torch.full((2 * n + 1, 2), -JUNK, dtype=torch.int32, device=DEV)]
    for log in logs:                                                          # two calls of everything: equal bits
        for k, (row, prev, size, hold) in enumerate(cases):
            roi.track(rows[k], None if prev is None else prevs[k], log[2 * k + 1], size, H, W, hold)
    got, again = (log.cpu().numpy() for log in logs)
    assert (got[0::2] == JUNK).all() and (again[0::2] == -JUNK).all()         # the rows between are not disturbed
    assert np.array_equal(got[1::2], again[1::2])
    for k, (row, prev, (h, w), hold) in enumerate(cases):
        want = TR.track_row(row, prev, h, w, H, W, hold)
        assert tuple(got[2 * k + 1]) == want, (row, prev, (h, w), hold, got[2 * k + 1], want)
        box = row[4:] if prev is None or TR.empty(row[4:]) else (row[4] + prev[0], row[5] + prev[1], row[6] + prev[0], row[7] + prev[1])
        assert want == roi.track_origin(box, prev, h, w, H, W, hold)          # the host policy says the same
        assert 0 <= want[0] <= H - h and 0 <= want[1] <= W - w


def test_track_clamps_a_previous_origin_outside_the_frame(lib):
    from otvm_amd import roi
    H, W, h, w = 33, 70, 16, 35
    rows = dev(np.array([[0, 0, 0, 0, 5, 9, 9, 20], [0, 0, 0, 0, h, w, -1, -1]], np.int32))
    for prev in ((-2, -2), (H - h + 2, W - w + 2), (-1, W - w + 1)):
        for k in range(2):
            out = torch.full((2,), JUNK, dtype=torch.int32, device=DEV)
            roi.track(rows[k], dev(np.array(prev, np.int32)), out, (h, w), H, W, 2)
            assert tuple(out.cpu().tolist()) == TR.track_row(rows[k].cpu().tolist(), prev, h, w, H, W, 2), (prev, k)
    with pytest.raises(ValueError, match="hold"):
        roi.track(rows[0], None, torch.zeros(2, dtype=torch.int32, device=DEV), (h, w), H, W, 0)
    with pytest.raises(ValueError, match="1 <= h <= 33"):
        roi.track(rows[0], None, torch.zeros(2, dtype=torch.int32, device=DEV), (34, w), H, W, 1)


# ------------------------------------------------------------------------------------------------ otvm_roi_crop_at / otvm_roi_paste_at
def _crop_at_raw(lib, origin, size, H, W, frame=None, trimap=None, labels=None):
    from otvm_amd import lib as L
    h, w = size
    p = L.RoiCropParams()
    p.H, p.W, p.y0, p.x0, p.h, p.w = H, W, 12345, -6789, h, w                  # (y0, x0 of the struct are not looked at)
    outs = (None if frame is None else torch.full((h, w, 3), 77, dtype=torch.uint8, device=DEV),
            None if trimap is None else torch.full((3, h, w), -7.0, dtype=torch.float32, device=DEV),
            None if labels is None else torch.full((h, w), 77, dtype=torch.uint8, device=DEV))
    for name, src, dst in zip(("frame", "trimap", "labels"), (frame, trimap, labels), outs):
        setattr(p, name, None if src is None else src.data_ptr())
        setattr(p, name + "_out", None if dst is None else dst.data_ptr())
    rc = lib.otvm_roi_crop_at(C.byref(p), origin.data_ptr(), stream())
    torch.cuda.synchronize()
    return (rc,) + outs


def _paste_at_raw(lib, origin, size, H, W, alpha, tri, fgr=None, frame=None, rgb=0, outside=None, want=("alpha", "alpha_u8", "trimap", "fgr")):
    from otvm_amd import lib as L
    h, w = size
    p = L.RoiPasteParams()
    p.H, p.W, p.y0, p.x0, p.h, p.w, p.u8_rgb = H, W, -4321, 99999, h, w, rgb
    p.win_alpha, p.win_trimap = alpha.data_ptr(), tri.data_ptr()
    p.win_fgr = None if fgr is None else fgr.data_ptr()
    p.frame = None if frame is None else frame.data_ptr()
    p.outside = None if outside is None else outside.data_ptr()
    outs = {}
    for name, shape, dt, fill in (("alpha", (H, W), torch.float32, -7.0), ("alpha_u8", (H, W), torch.uint8, 77),
                                  ("trimap", (3, H, W), torch.float32, -7.0), ("fgr", (3, H, W), torch.float32, -7.0)):
        if name in want:
            outs[name] = torch.full(shape, fill, dtype=dt, device=DEV)
            setattr(p, name, outs[name].data_ptr())
    rc = lib.otvm_roi_paste_at(C.byref(p), origin.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, outs


ALL = ("alpha", "alpha_u8", "trimap", "fgr")


def _check_paste_at(lib, logged, win, H, W, frame, outside_np, rgb, with_fgr, want, seed):
    """The device-origin paste with ``logged`` in the log row against the host-origin paste at ``win`` and the restatement."""
    alpha, tri, fgr = _window_results(win[2], win[3], seed)
    ref = dict(zip(ALL, TR.paste_at(logged, win[2:], H, W, alpha, tri, fgr if with_fgr else None, frame, bool(rgb), outside_np)))
    args = (dev(alpha), dev(tri), dev(fgr) if with_fgr else None, dev(frame) if with_fgr else None, rgb,
            None if outside_np is None else dev(outside_np), want)
    rc, outs = _paste_at_raw(lib, dev(np.array(logged, np.int32)), win[2:], H, W, *args)
    rc0, outs0 = _paste_raw(lib, win, H, W, *args)
    what = (logged, win, H, W, rgb, with_fgr, outside_np is not None, want)
    assert rc == 0 and rc0 == 0 and sorted(outs) == sorted(want), what
    for name in want:
        assert np.array_equal(bits(outs[name]), bits(outs0[name])), what + (name, "host-origin kernel")
        assert np.array_equal(bits(outs[name]), bits(ref[name])), what + (name, "restatement")


@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_crop_at_and_paste_at_equal_the_host_origin_kernels(lib, H, W):
    frame, tri, lab = _frame_inputs(H, W, 13 * H + W)
    g = np.random.default_rng(W + 1)
    ocls = g.choice(3, size=(H, W))
    outside = np.stack([(ocls == k) for k in range(3)]).astype(np.float32)
    fd, td, ld = dev(frame), dev(tri), dev(lab)
    for j, win in enumerate(_windows(H, W)):
        y0, x0, h, w = win
        # the logged origin itself, and -- where the window lies against a side of the frame -- one 2 pixels beyond the legal range
        # on that side: the kernel clamps what it reads, so the result is the clamped origin's
        logged = [(y0, x0)]
        if y0 == 0 and x0 == 0:
            logged.append((-2, -2))
        if y0 == H - h and x0 == W - w:
            logged.append((H - h + 2, W - w + 2))
        if y0 == 0 and x0 == W - w:
            logged.append((-2, W - w + 2))
        for at in logged:
            o = dev(np.array(at, np.int32))
            wf, wt, wl = TR.crop_at(at, (h, w), H, W, frame, tri, lab)
            rc0, hf, ht, hl = _crop_raw(lib, win, H, W, fd, td, ld)
            rc, gf, gt, gl = _crop_at_raw(lib, o, (h, w), H, W, fd, td, ld)
            assert rc == 0 and rc0 == 0, (win, at)
            assert torch.equal(gf, hf) and np.array_equal(bits(gt), bits(ht)) and torch.equal(gl, hl), (win, at)
            assert np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(bits(gt), bits(wt)) and np.array_equal(gl.cpu().numpy(), wl), (win, at)
            # each destination alone
            assert np.array_equal(_crop_at_raw(lib, o, (h, w), H, W, frame=fd)[1].cpu().numpy(), wf), (win, at)
            assert np.array_equal(bits(_crop_at_raw(lib, o, (h, w), H, W, trimap=td)[2]), bits(wt)), (win, at)
            assert np.array_equal(_crop_at_raw(lib, o, (h, w), H, W, labels=ld)[3].cpu().numpy(), wl), (win, at)
            assert o.cpu().tolist() == list(at)                               # the log row is read, never written
            for rgb, out_np in ((0, None), (1, outside)):
                _check_paste_at(lib, at, win, H, W, frame, out_np, rgb, True, ALL, 100 * j + rgb)
            _check_paste_at(lib, at, win, H, W, frame, outside, 0, False, ("alpha", "alpha_u8", "trimap"), j)        # without F
        for absent in ALL:                                                    # each output absent
            _check_paste_at(lib, (y0, x0), win, H, W, frame, None, 1, True, tuple(n for n in ALL if n != absent), j)


def test_python_wrappers_crop_at_and_paste_at(lib):
    from otvm_amd import roi
    H, W, win = 33, 71, (1, 37, 32, 32)
    frame, tri, lab = _frame_inputs(H, W, 9)
    log = dev(np.array([[JUNK, JUNK], [1, 37], [JUNK, JUNK]], np.int32))
    gf, gt, gl = roi.crop_at(log[1], (32, 32), frame=dev(frame), trimap=dev(tri), labels=dev(lab))
    hf, ht, hl = roi.crop(win, frame=dev(frame), trimap=dev(tri), labels=dev(lab))
    assert torch.equal(gf, hf) and np.array_equal(bits(gt), bits(ht)) and torch.equal(gl, hl)
    alpha, wtri, fgr = _window_results(32, 32, 1)
    got = roi.paste_at(log[1], (32, 32), H, W, dev(alpha), dev(wtri), dev(fgr), dev(frame), rgb=True)
    for g_, w_ in zip(got, roi.paste(win, H, W, dev(alpha), dev(wtri), dev(fgr), dev(frame), rgb=True)):
        assert np.array_equal(bits(g_), bits(w_))
    with pytest.raises(ValueError, match="1 <= w <= 71"):
        roi.crop_at(log[1], (32, 72), frame=dev(frame))
    with pytest.raises(ValueError, match="2 contiguous int32"):
        roi.crop_at(log[:, 0], (32, 32), frame=dev(frame))
    with pytest.raises(ValueError, match="2 contiguous int32"):
        roi.paste_at(log[1].long(), (32, 32), H, W, dev(alpha), dev(wtri))


# ------------------------------------------------------------------------------------------------ the route
H_, W_, T_, BAND, MARGIN = 160, 224, 8, 6, 16
KW = dict(skip=3, max_num=3)


def _disc_clip(dy, dx):
    """Eight frames of the synthetic clip, a soft disc of radius 20 centred at (40 + dy t, 48 + dx t), its trimap and its FULLY
    labelled label map (the band is label 1) per frame."""
    from otvm_amd.synth_data import synthetic_clip
    frames, _ = synthetic_clip(H_, W_, T_, seed=29)
    yy, xx = np.mgrid[0:H_, 0:W_]
    ms = [np.floor(np.clip((20 - np.sqrt((yy - 40 - dy * t) ** 2 + (xx - 48 - dx * t) ** 2)) / 3.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)
          for t in range(T_)]
    return ([np.ascontiguousarray(f) for f in frames], ms, [MR.trimap_from_mask(m, BAND) for m in ms],
            [MR.labels_from_mask(m, BAND, band_label=1) for m in ms])


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
        yield (_fresh_model(synth_sd, 12, "f16x3"),) + _disc_clip(9, 14)
    finally:
        engine.AUTOTUNE = old_auto
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


class _ExactTrimaps(torch.nn.Module):
    """The model with the trimap it RETURNS made exact: the one-hot of the step's label map, the step's own trimap on a keyframe.
    What the engine returns as out[1] is the alpha network's refined trimap -- the labels act on its input -- and the synthetic
    weights fill it with noise whose box is the whole window, so a window that follows it never moves.  With a trained model
    that trimap carries the subject; here the double puts the subject's classes where the labels say they are, on both sides
    of every comparison, so that the windows are known and move.  Everything else -- alpha, the bank, the schedule -- is the
    network's own, run in windows at different origins."""

    def __init__(self, model):
        super().__init__()
        self.module = model.module if hasattr(model, "module") else model

    def forward(self, *a, **kw):
        out = list(self.module(*a, **kw))
        if kw.get("labels") is not None:
            lab = kw["labels"]
            out[1] = torch.stack([(lab == k) for k in range(3)]).float()[None, None].contiguous()
        elif kw.get("first_frame") or kw.get("keyframe"):
            out[1] = kw["tri_gt"].clone()
        return tuple(out)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a.contiguous()), bits(b.contiguous()))


def _inside(x, win):
    y0, x0, h, w = win
    return x[..., y0:y0 + h, x0:x0 + w]


def _outside_mask(win):
    m = np.ones((H_, W_), bool)
    m[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = False
    return torch.from_numpy(m)


def _host_cropped(m, frames, wins, sources, **kw):
    """The definition: run_video_matte on the clip whose frame t and source t are cropped ON THE HOST at window t."""
    from otvm_amd.video import run_video_matte
    cropped = [R.crop(wins[t], frame=frames[t])[0] for t in range(len(frames))]
    kf = {t: (R.crop(wins[t], trimap=v)[1] if v.ndim == 3 else R.crop(wins[t], labels=v)[2]) for t, v in sources.items()}
    return run_video_matte(m, cropped, keyframes=kf, **KW, **kw)


def _check_by_definition(got, want, wins):
    for t, win in enumerate(wins):
        for k in ("alpha", "alpha_u8", "trimap"):
            assert _eq(_inside(got[k][t], win), want[k][t]), (k, t)
        out = _outside_mask(win)
        assert (got["alpha"][t][out] == 0).all() and (got["alpha_u8"][t][out] == 0).all(), t
        assert (got["trimap"][t][0][out] == 1).all() and (got["trimap"][t][1:][:, out] == 0).all(), t
    assert got["bank_frames"] == want["bank_frames"]


def _follows_the_policy(got, size, hold, k0=0, keys=()):
    """Every window that has no trimap of its own is the host policy applied to its neighbour's returned trimap and window."""
    from otvm_amd import roi
    for t in range(len(got["roi"])):
        if t in keys:
            continue
        n = TR.neighbour(t, k0)
        box = tuple(int(v) for v in R.bbox(got["trimap"][n].numpy())[4:])    # pasted: background outside, so this is the box inside
        assert got["roi"][t] == roi.track_origin(box, got["roi"][n][:2], size[0], size[1], H_, W_, hold) + size, t


def test_route_with_label_maps_by_definition(route):
    """The first frame has its trimap, every later frame a fully labelled label map, and the returned trimaps are exact
    (_ExactTrimaps): the windows are the restatement's -- 96x96, hold 8, seven distinct origins from (0, 0) to (37, 84) -- and
    the result is the matte of the clip cropped on the host at those windows, slots memorised from windows at different origins."""
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    m = _ExactTrimaps(m)
    sources = {0: tris[0], **{t: labs[t] for t in range(1, T_)}}
    got = run_video_matte(m, frames, trimap=tris[0], keyframes={t: labs[t] for t in range(1, T_)}, roi="track", roi_margin=MARGIN, **KW)
    wins, clipped = TR.clip_windows((96, 96), H_, W_, 8, range(T_), {0: tris[0]}, 0, [tris[0]] + labs[1:])
    wins = [wins[t] for t in range(T_)]
    assert got["roi"] == wins and got["roi_size"] == (96, 96) and got["roi_clipped"] == [] == clipped
    assert len({w[:2] for w in wins}) == 7 and wins[0][:2] == (0, 0) and wins[-1][:2] == (37, 84)
    assert tuple(got["alpha"].shape) == (T_, H_, W_) and tuple(got["trimap"].shape) == (T_, 3, H_, W_)
    want = _host_cropped(m, frames, wins, sources)
    _check_by_definition(got, want, wins)
    assert got["schedule"] == want["schedule"]
    assert any(len(b) > 1 for b in got["bank_frames"])                       # slots memorised from windows at different origins
    _follows_the_policy(got, (96, 96), 8, keys=(0,))
    # the output trimaps are exact: the label maps, where the window shows them
    for t in range(1, T_):
        assert np.array_equal(_inside(got["trimap"][t], wins[t]).numpy(), MR.onehot(R.crop(wins[t], labels=labs[t])[2])), t


def test_route_without_label_maps_follows_what_the_network_put_out(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    got = run_video_matte(m, frames, trimap=tris[0], roi="track", roi_margin=MARGIN, **KW)
    size = got["roi_size"]
    assert size == R.window_size([tuple(R.bbox(tris[0])[4:])], H_, W_, MARGIN)
    assert got["roi"][0] == R.window_origin(tuple(R.bbox(tris[0])[4:]), size[0], size[1], H_, W_) + size
    _follows_the_policy(got, size, 8, keys=(0,))
    cropped = [R.crop(got["roi"][t], frame=frames[t])[0] for t in range(T_)]
    want = run_video_matte(m, cropped, trimap=R.crop(got["roi"][0], trimap=tris[0])[1], **KW)
    _check_by_definition(got, want, got["roi"])
    assert "schedule" not in got


def test_the_frame_loop_reads_nothing_back(route, monkeypatch):
    from otvm_amd import roi
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    events, real = [], roi.rows_of

    def counted(buf):
        events.append("read")
        return real(buf)

    def never(rows):
        raise AssertionError("the tracking window reads back through roi.rows_of alone")
    monkeypatch.setattr(roi, "rows_of", counted)
    monkeypatch.setattr(roi, "boxes_of", never)
    got = run_video_matte(m, frames, trimap=tris[0], keyframes={5: labs[5]}, roi="track", roi_margin=MARGIN, keep_on_device=True,
                          on_frame=lambda i, a, u8, out: events.append(i), **KW)
    assert events == ["read"] + list(range(T_)) + ["read"]
    assert len(got["roi"]) == T_


def test_roi_clipped_lists_a_subject_that_outruns_the_window(route):
    from otvm_amd.video import run_video_matte
    m = _ExactTrimaps(route[0])
    frames, ms, tris, labs = _disc_clip(11, 17)
    got = run_video_matte(m, frames, trimap=tris[0], keyframes={t: labs[t] for t in range(1, T_)}, roi="track", roi_margin=MARGIN, **KW)
    wins, clipped = TR.clip_windows((96, 96), H_, W_, 8, range(T_), {0: tris[0]}, 0, [tris[0]] + labs[1:])
    assert got["roi"] == [wins[t] for t in range(T_)]
    assert got["roi_clipped"] == clipped == [4, 6]                            # first cut on frame 4: the held y axis lags two frames


def test_backward_sweep_follows_the_later_frame(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    sources = {3: tris[3], 1: labs[1], 6: tris[6]}
    got = run_video_matte(m, frames, keyframes=sources, roi="track", roi_margin=MARGIN, **KW)
    size = got["roi_size"]
    assert size == R.window_size([tuple(R.bbox(v)[4:]) for v in sources.values()], H_, W_, MARGIN)
    assert got["roi"][3] == R.window_origin(tuple(R.bbox(tris[3])[4:]), size[0], size[1], H_, W_) + size
    assert got["roi"][6] == R.window_origin(tuple(R.bbox(tris[6])[4:]), size[0], size[1], H_, W_) + size != got["roi"][3]
    assert [s[0] for s in got["schedule"]] == [3, 6, 4, 5, 7, 2, 1, 0]
    _follows_the_policy(got, size, 8, k0=3, keys=(3, 6))                     # 7 leans on 6; 2, 1, 0 lean on 3, 2, 1
    want = _host_cropped(m, frames, got["roi"], sources)
    _check_by_definition(got, want, got["roi"])
    assert got["schedule"] == want["schedule"] and got["anchor_frames"] == want["anchor_frames"]


def test_foreground_bytes_are_made_from_the_pasted_planes(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    eng, seen = m.module, {}

    def keep(i, alpha, u8, out):
        seen[i] = (out[3][0, 0, 0].cpu().numpy(), out[1][0, 0].cpu().numpy(), eng._engine.last_fgr.cpu().numpy())
    colour = (10, 200, 30)
    got = run_video_matte(m, frames[:4], trimap=tris[0], roi="track", roi_margin=MARGIN, foreground=True, new_background=colour,
                          on_frame=keep, **KW)
    assert torch.equal(got["fgr_u8"][..., 3], got["alpha_u8"]) and m.module.foreground is False
    for t, win in enumerate(got["roi"]):
        a_w, t_w, f_w = seen[t]
        assert a_w.shape == win[2:] and f_w.shape == (3,) + win[2:]
        alpha, u8, tri, F = R.paste(win, H_, W_, a_w, t_w, f_w, frames[t], False, None)
        _, rgba, comp = fgr_ref.fgr_outputs(alpha, F, colour, u8_rgb=False)
        assert np.array_equal(got["fgr_u8"][t].numpy(), rgba) and np.array_equal(got["comp_u8"][t].numpy(), comp), t
        assert np.array_equal(got["alpha_u8"][t].numpy(), u8) and np.array_equal(bits(got["alpha"][t]), bits(alpha)), t
        assert np.array_equal(bits(got["trimap"][t]), bits(tri)), t


def test_stabiliser_runs_behind_the_paste(route):
    from otvm_amd.temporal import TemporalStabiliser
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    kw = dict(trimap=tris[0], keyframes={t: labs[t] for t in range(1, T_)}, roi="track", roi_margin=MARGIN, **KW)
    got = run_video_matte(m, frames, stabilise=True, **kw)
    plain = run_video_matte(m, frames, **kw)
    assert _eq(got["alpha_raw"], plain["alpha"]) and _eq(got["trimap"], plain["trimap"]) and got["roi"] == plain["roi"]
    st = TemporalStabiliser(DEV, H_, W_)
    outs = [st.step(dev(frames[t]), got["alpha_raw"][t].to(DEV), trimap=got["trimap"][t].to(DEV), tri_scale=1, rgb=False) for t in range(T_)]
    assert _eq(got["alpha"], torch.stack([o[0] for o in outs]).cpu()) and _eq(got["alpha_u8"], torch.stack([o[1] for o in outs]).cpu())


def test_a_size_of_the_callers(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, labs = route
    m = _ExactTrimaps(m)
    sources = {0: tris[0], **{t: labs[t] for t in range(1, T_)}}
    got = run_video_matte(m, frames, trimap=tris[0], keyframes={t: labs[t] for t in range(1, T_)}, roi=("track", 128, 128),
                          roi_margin=MARGIN, **KW)
    wins, clipped = TR.clip_windows((128, 128), H_, W_, 8, range(T_), {0: tris[0]}, 0, [tris[0]] + labs[1:])
    assert got["roi"] == [wins[t] for t in range(T_)] and got["roi_size"] == (128, 128) and got["roi_clipped"] == clipped
    _check_by_definition(got, _host_cropped(m, frames, got["roi"], sources), got["roi"])
    with pytest.raises(ValueError, match="does not hold the trimap / label map of frame 0"):
        run_video_matte(m, frames, trimap=tris[0], roi=("track", 32, 128), **KW)


# ------------------------------------------------------------------------------------------------ eval_cli
def test_eval_cli_roi_track(tmp_path, route):
    import json
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames_bgr, ms, tris, labs = route
    demo = os.path.join(str(tmp_path), "demo")
    for sub in ("frames", "mask"):
        os.makedirs(os.path.join(demo, "clip", sub))
    for t in range(T_):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
    Image.fromarray(ms[0]).save(os.path.join(demo, "clip", "mask", "0000.png"))
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "3", "--mask-band", str(BAND)]
    out, sj = os.path.join(str(tmp_path), "out"), os.path.join(str(tmp_path), "s.json")
    res = eval_cli.main(common + ["--out", out, "--masks", "key", "--roi", "track", "--roi-margin", str(MARGIN), "--summary-json", sj])
    assert res["frames"] == T_
    s = json.load(open(sj))
    ref = run_video_matte(m, frames_bgr, keyframes={0: Mask(ms[0], band=BAND)}, roi="track", roi_margin=MARGIN, skip=3, max_num=5)
    assert s["roi"] == "track" and s["roi_margin"] == MARGIN and s["roi_size"] == {"clip": list(ref["roi_size"])}
    assert s["roi_clipped"] == {"clip": ref["roi_clipped"]}
    for t in range(T_):
        a = np.asarray(Image.open(os.path.join(out, "alpha", "test", "s4_OTVM", "pred", "clip", "%04d.png" % t)))
        assert np.array_equal(a, ref["alpha_u8"][t].numpy()), t
    with pytest.raises(SystemExit, match="--masks"):
        eval_cli.main(common + ["--out", out, "--masks", "frame", "--roi", "track"])
