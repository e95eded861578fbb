"""GPU (-m gpu): trimaps from segmentation masks -- otvm_trimap_from_mask against its numpy restatement
(tests/mask_trimap_ref.py) bit for bit on every size-selected path, determinism and refusals, and the routes through
run_video_matte (mask=, keyframes={t: Mask}, masks=) and eval_cli --masks against the same calls fed the restatement's arrays."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mask_trimap_cases as K
from tests import mask_trimap_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    from otvm_amd import lib
    lib.load()
    return gpu_util


def dev(G, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.DEV)


def _call(G, mask_d, H, W, lo, hi, t_fg, t_bg, want_trimap, want_labels, band_label=1, ws=None, fill=None):
    """One otvm_trimap_from_mask call on fresh (or pre-filled) outputs -> (rc, trimap or None, labels or None)."""
    from otvm_amd import lib as L
    lib = L.load()
    if ws is None:
        ws = torch.empty(max(2, lib.otvm_trimap_from_mask_ws_bytes(H, W)), dtype=torch.uint8, device=G.DEV)
    tri = torch.full((3, max(H, 1), max(W, 1)), -7.0 if fill is None else fill, dtype=torch.float32, device=G.DEV) if want_trimap else None
    lab = torch.full((max(H, 1), max(W, 1)), 77, dtype=torch.uint8, device=G.DEV) if want_labels else None
    p = L.MaskTrimapParams()
    p.mask, p.H, p.W, p.lo, p.hi, p.t_fg, p.t_bg, p.band_label = mask_d.data_ptr(), H, W, lo, hi, t_fg, t_bg, band_label
    p.trimap = tri.data_ptr() if tri is not None else None
    p.labels = lab.data_ptr() if lab is not None else None
    rc = lib.otvm_trimap_from_mask(C.byref(p), ws.data_ptr(), G.stream())
    torch.cuda.synchronize()
    return rc, tri, lab


def _masks_of(H, W):
    out = [("soft-%d-%d" % th, K.soft_mask(H, W, 5 * H + W + i), th) for i, th in enumerate(K.THRESHOLDS)]
    out += [("all-0", np.zeros((H, W), np.uint8), (127, 128)), ("all-255", np.full((H, W), 255, np.uint8), (127, 128)),
            ("one-fg", K.one_pixel(H, W, 255), (127, 128)), ("one-bg", K.one_pixel(H, W, 0), (25, 230))]
    return out


@pytest.mark.parametrize("H,W", K.SIZES, ids=["%dx%d" % s for s in K.SIZES])
def test_kernel_equals_the_restatement(G, H, W):
    T = K.T_VALUES
    for name, m, (lo, hi) in _masks_of(H, W):
        md = dev(G, m)
        for j, t_fg in enumerate(T):
            t_bg = T[(j + 3) % len(T)]                                   # every value serves both sets, the two differ
            cls = R.classes(m, lo, hi, t_fg, t_bg)
            w_tri = R.onehot(cls)
            what = (name, lo, hi, t_fg, t_bg)
            for want_trimap, want_labels, band_label in ((True, False, 1), (False, True, 1), (False, True, 255), (True, True, 255)):
                rc, tri, lab = _call(G, md, H, W, lo, hi, t_fg, t_bg, want_trimap, want_labels, band_label)
                assert rc == 0, what
                if want_trimap:
                    got = tri.cpu().numpy()
                    assert np.array_equal(got.view(np.uint32), w_tri.view(np.uint32)), what
                    assert ((got == 1.0).sum(0) == 1).all() and ((got == 0.0) | (got == 1.0)).all(), what    # one plane is 1.f
                if want_labels:
                    assert np.array_equal(lab.cpu().numpy(), R.label_map(cls, band_label)), what + (band_label,)


def test_kernel_equals_the_restatement_at_1080p_every_element(G):
    H, W, r = 1080, 1920, 20
    m = K.soft_mask(H, W, 9)
    m[300:800, 500:1500] = 255                                           # a deep interior: pixels farther than r from any edge
    m[0:200, 0:700] = 0
    rc, tri, lab = _call(G, dev(G, m), H, W, 127, 128, R.band_t(r), R.band_t(r), True, True, 255)
    assert rc == 0
    cls = R.classes(m, 127, 128, R.band_t(r), R.band_t(r))
    assert (cls == 0).any() and (cls == 1).any() and (cls == 2).any()
    assert np.array_equal(tri.cpu().numpy().view(np.uint32), R.onehot(cls).view(np.uint32))
    assert np.array_equal(lab.cpu().numpy(), R.label_map(cls, 255))


def test_python_wrapper_float_masks_and_bands(G):
    from otvm_amd import masks
    H, W = 70, 129
    g = np.random.default_rng(3)
    soft = np.clip(np.kron(g.random((H // 10 + 1, W // 10 + 1)), np.ones((10, 10)))[:H, :W] * 1.4 - 0.2, -0.1, 1.1).astype(np.float32)
    for band, lo, hi in ((5, 127, 128), ((3.5, 12), 25, 230), (0, 127, 128)):
        got = masks.trimap_from_mask(dev(G, soft), band, lo, hi)
        lab = masks.trimap_from_mask(dev(G, soft), band, lo, hi, labels=True, band_label=255)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, H, W) and lab.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.trimap_from_mask(soft, band, lo, hi))
        assert np.array_equal(lab.cpu().numpy(), R.labels_from_mask(soft, band, lo, hi, 255))
    u8 = R.quantise(soft)
    assert torch.equal(masks.trimap_from_mask(dev(G, u8), 5), masks.trimap_from_mask(dev(G, soft), 5))
    with pytest.raises(ValueError):
        masks.trimap_from_mask(torch.zeros(4, 4), 5)                     # not on the GPU
    with pytest.raises(ValueError):
        masks.trimap_from_mask(dev(G, u8), 256)
    with pytest.raises(ValueError):
        masks.trimap_from_mask(dev(G, u8), 5, lo=128, hi=128)
    with pytest.raises(ValueError):
        masks.trimap_from_mask(dev(G, u8), 5, labels=True, band_label=2)


def test_two_calls_give_equal_bits_and_bad_arguments_launch_nothing(G):
    from otvm_amd import lib as L
    lib = L.load()
    H, W = 135, 241
    m = K.soft_mask(H, W, 21)
    md = dev(G, m)
    ws = torch.empty(lib.otvm_trimap_from_mask_ws_bytes(H, W), dtype=torch.uint8, device=G.DEV)
    ws.fill_(0xAB)                                                       # the workspace needs no initialisation
    rc, a_tri, a_lab = _call(G, md, H, W, 25, 230, 400, 25, True, True, 1, ws=ws)
    ws.fill_(0x11)
    rc2, b_tri, b_lab = _call(G, md, H, W, 25, 230, 400, 25, True, True, 1, ws=ws)
    assert rc == 0 and rc2 == 0
    assert torch.equal(a_tri.view(torch.int32), b_tri.view(torch.int32)) and torch.equal(a_lab, b_lab)
    ok = dict(H=H, W=W, lo=25, hi=230, t_fg=400, t_bg=25, band_label=1)
    bad = [dict(H=0), dict(W=0), dict(H=16384), dict(W=16384), dict(H=-1), dict(lo=-1), dict(lo=230), dict(lo=231, hi=230), dict(hi=256),
           dict(t_fg=-1), dict(t_fg=65026), dict(t_bg=-1), dict(t_bg=65026), dict(band_label=0), dict(band_label=2), dict(band_label=254)]
    for change in bad:
        kw = dict(ok, **change)
        tri = torch.full((3, H, W), -7.0, device=G.DEV)
        lab = torch.full((H, W), 77, dtype=torch.uint8, device=G.DEV)
        p = L.MaskTrimapParams()
        p.mask, p.trimap, p.labels = md.data_ptr(), tri.data_ptr(), lab.data_ptr()
        for k, v in kw.items():
            setattr(p, k, v)
        rc = lib.otvm_trimap_from_mask(C.byref(p), ws.data_ptr(), G.stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.otvm_last_error().decode().startswith("otvm_trimap_from_mask"), change
        assert bool((tri == -7.0).all()) and bool((lab == 77).all()), change
    # null pointers, no output at all, a misaligned trimap
    for null in ("mask", "ws", "outputs", "params", "misaligned"):
        tri = torch.full((3 * H * W + 1,), -7.0, device=G.DEV)
        p = L.MaskTrimapParams()
        for k, v in ok.items():
            setattr(p, k, v)
        p.mask = None if null == "mask" else md.data_ptr()
        if null != "outputs":
            p.trimap = tri.data_ptr() + (2 if null == "misaligned" else 0)
        rc = lib.otvm_trimap_from_mask(None if null == "params" else C.byref(p), None if null == "ws" else ws.data_ptr(), G.stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.otvm_last_error().decode().startswith("otvm_trimap_from_mask"), null
        assert bool((tri == -7.0).all()), null


# ------------------------------------------------------------------------------------------------ routes
H_, W_, T_ = 100, 150, 6


def _clip_masks():
    """Six frames of the synthetic clip and a soft mask per frame that follows its moving disc (uint8, soft rim)."""
    from otvm_amd.synth_data import synthetic_clip
    frames, _ = synthetic_clip(H_, W_, T_, seed=53)
    yy, xx = np.mgrid[0:H_, 0:W_]
    ms = []
    for t in range(T_):
        r = np.sqrt((yy - H_ / 2 - 0.5 * t) ** 2 + (xx - W_ / 2 - 1.0 * t) ** 2)
        ms.append(np.floor(np.clip((H_ / 3.5 - r) / 3.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8))
    return frames, ms


@pytest.fixture(scope="module")
def route(G, synth_sd, tmp_path_factory):
    """One model for all route tests: the autotuner's choices (written once to a file) are shared by every call."""
    from tests.test_gpu_frame import _fresh_model
    old = os.environ.get("OTVM_TUNE_FILE")
    os.environ["OTVM_TUNE_FILE"] = os.path.join(str(tmp_path_factory.mktemp("tune")), "tune.json")
    frames, ms = _clip_masks()
    try:
        yield _fresh_model(synth_sd, 12, "f16x3"), frames, ms
    finally:
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


def _same(a, b, keys=("alpha", "alpha_u8", "trimap")):
    for k in keys:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8 if a[k].dtype == torch.uint8 else torch.int32),
                                                        b[k].view(torch.uint8 if b[k].dtype == torch.uint8 else torch.int32)), k
    assert a["bank_frames"] == b["bank_frames"]


def test_mask_equals_the_trimap_route(route):
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, ms = route
    kw = dict(skip=2, max_num=3)
    want = run_video_matte(m, frames, trimap=R.trimap_from_mask(ms[0], 12), **kw)                 # band: the model's DILATION_KERNEL
    _same(run_video_matte(m, frames, mask=ms[0], **kw), want)
    _same(run_video_matte(m, frames, mask=Mask(ms[0]), **kw), want)
    _same(run_video_matte(m, frames, mask=torch.from_numpy(ms[0]).float() / 255, **kw), want)     # a float mask: quantised back
    want2 = run_video_matte(m, frames, trimap=R.trimap_from_mask(ms[0], (4, 9.5), 25, 230), **kw)
    _same(run_video_matte(m, frames, mask=Mask(ms[0], band=(4, 9.5), lo=25, hi=230), **kw), want2)
    assert not torch.equal(want["alpha"], want2["alpha"])
    with pytest.raises(ValueError, match="100x150"):
        run_video_matte(m, frames, mask=ms[0][:50], **kw)


def test_keyframe_masks_equal_the_array_route(route):
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, ms = route
    kw = dict(skip=2, max_num=3)
    got = run_video_matte(m, frames, keyframes={0: Mask(ms[0], band=6), 3: Mask(ms[3], band=6), 4: Mask(ms[4], band=6, role="labels")}, **kw)
    want = run_video_matte(m, frames, keyframes={0: R.trimap_from_mask(ms[0], 6), 3: R.trimap_from_mask(ms[3], 6),
                                                 4: R.labels_from_mask(ms[4], 6, band_label=255)}, **kw)
    _same(got, want)
    assert got["schedule"] == want["schedule"] and got["anchor_frames"] == want["anchor_frames"]
    lab = R.labels_from_mask(ms[4], 6, band_label=255)
    assert (lab == 255).any() and (lab == 0).any() and (lab == 2).any()


def test_masks_route_mattes_every_frame_alone(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms = route
    core = m.module
    seen = []
    got = run_video_matte(m, frames, masks=ms, skip=2, max_num=3, on_frame=lambda i, a, u8, out: seen.append((i, core._engine.last_T_read)))
    assert got["bank_frames"] == [[]] * T_ and seen == [(i, 0) for i in range(T_)] and core._engine.last_T_read == 0
    assert sorted(got) == ["alpha", "alpha_u8", "bank_frames", "trimap"]
    for t in range(T_):
        one = run_video_matte(m, frames[t:t + 1], trimap=R.trimap_from_mask(ms[t], 12), skip=2, max_num=3)
        for k in ("alpha", "alpha_u8", "trimap"):
            assert torch.equal(got[k][t], one[k][0]), (k, t)
        assert one["bank_frames"] == [[]]
    with pytest.raises(ValueError, match="150"):
        run_video_matte(m, frames, masks=ms[:5] + [ms[5][:, :100]])


def test_mask_at_working_resolution_equals_the_trimap_route(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms = route
    kw = dict(skip=2, max_num=3, work_scale=2)
    got = run_video_matte(m, frames, mask=ms[0], **kw)
    want = run_video_matte(m, frames, trimap=R.trimap_from_mask(ms[0], 12), **kw)
    _same(got, want)
    assert got["work_size"] == want["work_size"] == (50, 75) and tuple(got["alpha"].shape) == (T_, H_, W_)
    per = run_video_matte(m, frames[:2], masks=ms[:2], **kw)
    for t in range(2):
        one = run_video_matte(m, frames[t:t + 1], trimap=R.trimap_from_mask(ms[t], 12), **kw)
        assert torch.equal(per["alpha_u8"][t], one["alpha_u8"][0]) and torch.equal(per["trimap"][t], one["trimap"][0])


def test_masks_route_with_foreground_and_metrics(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms = route
    got = run_video_matte(m, frames, masks=ms, foreground=True, new_background=(10, 200, 30), gt_alpha_u8=ms, gt_mask="unknown")
    assert tuple(got["fgr_u8"].shape) == (T_, H_, W_, 4) and tuple(got["comp_u8"].shape) == (T_, H_, W_, 3)
    assert torch.equal(got["fgr_u8"][..., 3], got["alpha_u8"])
    assert got["metrics"]["frames"] == T_ and got["bank_frames"] == [[]] * T_
    plain = run_video_matte(m, frames, masks=ms)
    assert torch.equal(plain["alpha_u8"], got["alpha_u8"]) and m.module.foreground is False


# ------------------------------------------------------------------------------------------------ eval_cli
def test_eval_cli_masks_key_and_frame(G, tmp_path, route):
    import json
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames_bgr, ms = route
    demo = os.path.join(str(tmp_path), "demo")
    for sub in ("frames", "mask"):
        os.makedirs(os.path.join(demo, "clip", sub))
    for t in range(T_):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
    for t in (1, 4):
        Image.fromarray(ms[t]).save(os.path.join(demo, "clip", "mask", "%04d.png" % t))
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "2"]

    def pngs(out, sub=None):
        d = os.path.join(out, "alpha", "test", "s4_OTVM", "pred", "clip") if sub is None else os.path.join(out, sub, "clip")
        return [np.asarray(Image.open(os.path.join(d, "%04d.png" % t))) for t in range(T_)]
    # key: the masks of frames 1 and 4 are full keyframes; frame 0 is reached by the backward sweep
    out, sj = os.path.join(str(tmp_path), "out_key"), os.path.join(str(tmp_path), "key.json")
    res = eval_cli.main(common + ["--out", out, "--masks", "key", "--mask-band", "6,9", "--mask-thresholds", "25,230", "--fgr",
                                  "--summary-json", sj])
    assert res["frames"] == T_
    s = json.load(open(sj))
    assert s["masks"] == "key" and s["mask_band"] == [6.0, 9.0] and s["mask_thresholds"] == [25, 230]
    ref = run_video_matte(m, frames_bgr, keyframes={t: Mask(ms[t], band=(6, 9), lo=25, hi=230) for t in (1, 4)}, skip=2, max_num=5,
                          foreground=True)
    for t, (a, f) in enumerate(zip(pngs(out), pngs(out, "fgr"))):
        assert np.array_equal(a, ref["alpha_u8"][t].numpy()), t
        assert np.array_equal(f, ref["fgr_u8"][t].numpy()[..., [2, 1, 0, 3]]), t          # the PNG is RGBA, the frames were BGR
    # frame: every frame needs its mask
    with pytest.raises(SystemExit, match="every frame"):
        eval_cli.main(common + ["--out", out, "--masks", "frame"])
    for t in (0, 2, 3, 5):
        Image.fromarray(ms[t]).save(os.path.join(demo, "clip", "mask", "%04d.png" % t))
    out, sj = os.path.join(str(tmp_path), "out_frame"), os.path.join(str(tmp_path), "frame.json")
    eval_cli.main(common + ["--out", out, "--masks", "frame", "--summary-json", sj])
    s = json.load(open(sj))
    assert s["masks"] == "frame" and s["mask_band"] == [12, 12] and s["mask_thresholds"] == [127, 128]
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames_bgr]
    ref = run_video_matte(m, rgb, masks=ms, skip=2, max_num=5, frames_are_rgb=True)
    for t, a in enumerate(pngs(out)):
        assert np.array_equal(a, ref["alpha_u8"][t].numpy()), t
    # a trimap file and a mask file on one frame; no mask folder use without --demo; lock-step batches
    os.makedirs(os.path.join(demo, "clip", "trimap"))
    Image.fromarray(np.where(ms[1] > 128, 255, 0).astype(np.uint8)).save(os.path.join(demo, "clip", "trimap", "0001.png"))
    with pytest.raises(SystemExit, match="mask AND a trimap"):
        eval_cli.main(common + ["--out", out, "--masks", "key", "--keyframes"])
    with pytest.raises(SystemExit, match="--batch"):
        eval_cli.main(common + ["--out", out, "--masks", "key", "--batch", "2"])
    with pytest.raises(SystemExit, match="--demo"):
        eval_cli.main(["--data", demo, "--synthetic-weights", "--out", out, "--masks", "key"])
