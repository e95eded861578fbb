"""GPU (-m gpu): working-resolution matting -- the reductions, the guided-filter coefficients and the full-resolution apply
against their numpy restatement (tests/guided_ref.py) bit for bit, the filter's two properties on the device output, and the
route through run_video_matte / eval_cli."""
import os

import numpy as np
import pytest
import torch

from tests import fgr_ref
from tests import guided_cases as K
from tests import guided_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    from otvm_amd import lib
    lib.load()
    return gpu_util


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def dev(G, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.DEV)


# ------------------------------------------------------------------------------------------------ reductions
def _trimap(g, H, W):
    cls = g.integers(0, 3, (H // 6 + 1, W // 6 + 1)).repeat(6, 0).repeat(6, 1)[:H, :W]      # 6 x 6 patches: solid blocks exist
    tri = np.stack([(cls == k) for k in range(3)]).astype(np.float32)
    soft = g.random((H, W)) < 0.02
    tri[2][soft & (cls == 2)] = np.float32(0.999)            # nearly-one is not one
    return tri


def _labels(g, H, W):
    lab = g.integers(0, 3, (H // 5 + 1, W // 5 + 1)).repeat(5, 0).repeat(5, 1)[:H, :W].astype(np.uint8)
    lab[g.random((H, W)) < 0.03] = 255
    lab[g.random((H, W)) < 0.01] = 7
    lab[: H // 3, : W // 3] = 255
    return lab


RED_CASES = [(37, 53, 2), (37, 53, 3), (37, 53, 4), (5, 7, 2), (5, 7, 3), (5, 7, 4), (1080, 1920, 2)]


@pytest.mark.parametrize("H,W,s", RED_CASES, ids=["%dx%d-s%d" % c for c in RED_CASES])
def test_reductions_equal_the_restatement(G, H, W, s):
    from otvm_amd import guided
    g = np.random.default_rng(H * 3 + W + s)
    img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[: H // 2, : W // 2] = 255                            # saturated blocks: the sum must not wrap
    tri, lab = _trimap(g, H, W), _labels(g, H, W)
    got = (guided.downsample_u8(dev(G, img), s), guided.downsample_trimap(dev(G, tri), s), guided.downsample_labels(dev(G, lab), s))
    torch.cuda.synchronize()
    want = (R.downsample_u8(img, s), R.downsample_trimap(tri, s), R.downsample_labels(lab, s))
    for name, a, b in zip(("u8", "trimap", "labels"), got, want):
        a = a.cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(bits(a), bits(b)), name


# ------------------------------------------------------------------------------------------------ coefficients
def _guide(g, h, w, constant):
    guide = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if constant:
        guide[:, : w // 2] = (90, 200, 17)                   # singular covariance on the left: eps alone conditions the solve
    return guide


def _targets(g, C, h, w):
    t = g.random((C, h, w), dtype=np.float32)
    t[:, : h // 2, : w // 3] = 1.0
    t[:, h // 2:, : w // 3] = 0.0
    t[0, 0, -1], t[0, -1, -1] = np.float32(1.5), np.float32(-0.25)       # clamped by the quantisation
    return t


COEF_SIZES = [(5, 7), (37, 53), (70, 100)]


@pytest.mark.parametrize("eps", [1e-6, 1e-2], ids=["eps1e-6", "eps1e-2"])
@pytest.mark.parametrize("r", [1, 4], ids=["r1", "r4"])
@pytest.mark.parametrize("C", [1, 4], ids=["C1", "C4"])
@pytest.mark.parametrize("h,w", COEF_SIZES, ids=["%dx%d" % c for c in COEF_SIZES])
def test_coefficients_equal_the_restatement(G, h, w, C, r, eps):
    from otvm_amd.guided import GuidedUpsampler
    for constant in (True, False):
        g = np.random.default_rng(h * 11 + w + C + r + int(constant))
        guide, tg = _guide(g, h, w, constant), _targets(g, C, h, w)
        ups = GuidedUpsampler(G.DEV, 2 * h, 2 * w, 2, r, eps, C)
        ups.coeffs(dev(G, guide), list(dev(G, tg)))
        torch.cuda.synchronize()
        raw, mean = ups.coef_raw.cpu().numpy(), ups.coef.cpu().numpy()
        w_raw, w_mean = R.guided_coeffs(guide, tg, r, eps)
        assert np.isfinite(raw).all() and np.isfinite(mean).all()
        assert np.array_equal(bits(raw), bits(w_raw)), "raw coefficients (constant region: %s)" % constant
        assert np.array_equal(bits(mean), bits(w_mean)), "mean coefficients (constant region: %s)" % constant


# ------------------------------------------------------------------------------------------------ apply
def _apply_case(G, H, W, s, C, r=2, eps=1e-4, seed=0):
    from otvm_amd.guided import GuidedUpsampler
    g = np.random.default_rng(seed + H + W + s)
    frame = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ups = GuidedUpsampler(G.DEV, H, W, s, r, eps, C)
    fd = dev(G, frame)
    wf = ups.reduce(fd)
    tg = _targets(g, C, ups.h, ups.w)
    tg[:, :, ups.w // 3:] *= np.float32(1.4)                 # some targets above one: the apply's clamp works
    ups.coeffs(wf, list(dev(G, tg)))
    a, u8, F = ups.apply(fd)
    torch.cuda.synchronize()
    coef = ups.coef.cpu().numpy()                            # the device's own coefficients
    w_a, w_u8, w_F = R.guided_apply(frame, coef, s)
    assert np.array_equal(bits(a.cpu().numpy()), bits(w_a))
    assert np.array_equal(u8.cpu().numpy(), w_u8)
    if C == 4:
        assert np.array_equal(bits(F.cpu().numpy()), bits(w_F))
    else:
        assert F is None
    return w_a


@pytest.mark.parametrize("C", [1, 4], ids=["C1", "C4"])
@pytest.mark.parametrize("s", [2, 3, 4], ids=["s2", "s3", "s4"])
@pytest.mark.parametrize("H,W", [(73, 105), (140, 200)], ids=["105x73", "200x140"])
def test_apply_equals_the_restatement(G, H, W, s, C):
    a = _apply_case(G, H, W, s, C)
    assert 0.0 <= a.min() and a.max() <= 1.0 and (a == 1.0).any() and ((a > 0) & (a < 1)).any()


def test_apply_equals_the_restatement_at_4k_every_element(G):
    _apply_case(G, 2160, 3840, 2, 1)


def test_apply_refuses_bad_arguments(G):
    import ctypes as C
    from otvm_amd import lib as L
    from otvm_amd.guided import GuidedUpsampler
    lib = L.load()
    ups = GuidedUpsampler(G.DEV, 10, 14, 2, 1, 1e-4, 1)
    p = ups._params()
    p.guide_work, p.target[0] = ups.coef.data_ptr(), ups.coef.data_ptr()
    for field, bad in (("s", 5), ("r", 0), ("r", 5), ("C", 2), ("h", 6), ("eps", 0.0)):
        q = ups._params()
        q.guide_work, q.target[0] = p.guide_work, p.target[0]
        setattr(q, field, bad)
        assert lib.otvm_guided_coeffs(C.byref(q), ups.ws.data_ptr(), G.stream()) != 0, field
    q = ups._params()
    q.guide_full, q.alpha, q.C = ups.coef.data_ptr(), ups.coef.data_ptr(), 4     # four targets without the F planes
    assert lib.otvm_guided_apply(C.byref(q), G.stream()) != 0


def test_apply_scalar_path_and_nan_select(G):
    """W % 4 == 0 with outputs that are only 4-byte aligned takes the pixel-by-pixel path: equal bits to the 16-byte path.  And a
    NaN coefficient gives 0 (alpha and byte), as the restatement has it."""
    import ctypes as C
    from otvm_amd import lib as L
    from otvm_amd.guided import GuidedUpsampler
    lib = L.load()
    H, W, s = 38, 52, 2
    g = np.random.default_rng(77)
    frame = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ups = GuidedUpsampler(G.DEV, H, W, s, 2, 1e-4, 4)
    fd = dev(G, frame)
    ups.coeffs(ups.reduce(fd), list(dev(G, _targets(g, 4, ups.h, ups.w))))
    ups.coef[3, 5, 0, 1] = float("nan")
    ups.coef[7, 2, 2, 3] = float("inf")
    a, u8, F = ups.apply(fd)
    buf_a = torch.full((H * W + 1,), -3.0, device=G.DEV)
    buf_f = torch.full((3 * H * W + 1,), -3.0, device=G.DEV)
    buf_u = torch.full((H * W + 1,), 9, dtype=torch.uint8, device=G.DEV)
    p = ups._params()
    p.guide_full, p.alpha, p.fgr = fd.data_ptr(), buf_a[1:].data_ptr(), buf_f[1:].data_ptr()
    p.alpha_u8 = buf_u[1:].data_ptr()
    L.check(lib.otvm_guided_apply(C.byref(p), G.stream()), "guided_apply")
    torch.cuda.synchronize()
    assert float(buf_a[0]) == -3.0 and float(buf_f[0]) == -3.0 and int(buf_u[0]) == 9
    assert torch.equal(buf_a[1:].view(torch.int32), a.flatten().view(torch.int32))
    assert torch.equal(buf_f[1:].view(torch.int32), F.flatten().view(torch.int32)) and torch.equal(buf_u[1:], u8.flatten())
    w_a, w_u8, w_F = R.guided_apply(frame, ups.coef.cpu().numpy(), s)
    assert np.array_equal(bits(a.cpu().numpy()), bits(w_a)) and np.array_equal(u8.cpu().numpy(), w_u8)
    assert np.array_equal(bits(F.cpu().numpy()), bits(w_F))
    assert not np.isnan(w_a).any() and (w_a[4:8, 8:12] == 0).any()


# ------------------------------------------------------------------------------------------------ properties, device output
def _device_upsample(G, frame, wf, alpha_w, s, r, eps):
    from otvm_amd.guided import GuidedUpsampler
    H, W = frame.shape[:2]
    ups = GuidedUpsampler(G.DEV, H, W, s, r, eps, 1)
    a, u8, _ = ups.upsample(dev(G, frame), dev(G, wf), [dev(G, alpha_w)])
    torch.cuda.synchronize()
    return a.cpu().numpy(), u8.cpu().numpy()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_device_output_keeps_solid_regions(G, s):
    """As tests/test_guided_cpu.py::test_restatement_keeps_solid_regions (the filter's support is 2r)."""
    frame, wf, al = K.solid_case(s=s)
    H, W = frame.shape[:2]
    for r in (1, 4):
        a, u8 = _device_upsample(G, frame, wf, al, s, r, 1e-4)
        for v in (0.0, 1.0):
            m = K.solid_mask(al, v, H, W, s, 2 * r)
            assert m.sum() > 300
            assert (a[m] == np.float32(v)).all() and (u8[m] == int(v * 255)).all()


def test_device_output_beats_bilinear_on_a_subpixel_edge(G):
    for s in (2, 3, 4):
        frame, true, wf, wa = K.edge_case(s=s)
        H, W = true.shape
        a, _ = _device_upsample(G, frame, wf, wa, s, 2, 1e-4)
        b = R.bilinear_upsample(wa, H, W, s)
        sg, sb = float(np.abs(a - true).sum()), float(np.abs(b - true).sum())
        print("guided margin s=%d r=2 eps=1e-4: device guided SAD %.3f, bilinear SAD %.3f, ratio %.3f" % (s, sg, sb, sg / sb))
        assert sg < sb


# ------------------------------------------------------------------------------------------------ end to end
def _clip_with_labels(H, W, T, seed):
    from otvm_amd.synth_data import synthetic_clip
    frames, tri = synthetic_clip(H, W, T, seed)
    lab = np.full((H, W), 255, np.uint8)
    lab[10:31, 20:45] = 2
    lab[50:77, 60:101] = 0
    lab[33:40, 5:18] = 1
    return frames, tri, lab


@pytest.mark.parametrize("skip", [2, 3], ids=["skip2", "skip3"])
def test_run_video_matte_at_working_resolution(G, synth_sd, tmp_path, monkeypatch, skip):
    from tests.test_gpu_frame import _fresh_model
    from otvm_amd.video import run_video_matte
    monkeypatch.setenv("OTVM_TUNE_FILE", os.path.join(str(tmp_path), "tune.json"))
    H, W, T, s, r, eps = 96, 128, 4, 2, 2, 1e-4
    frames, tri, lab = _clip_with_labels(H, W, T, seed=37)
    bg = np.random.default_rng(4).integers(0, 256, (H, W, 3), dtype=np.uint8)
    m = _fresh_model(synth_sd, 12, "f16x3")
    core = m.module
    kw = dict(skip=skip, max_num=3)
    before = run_video_matte(m, frames, trimap=tri, keyframes={2: lab}, **kw)
    work_alpha, work_fgr = {}, {}

    def grab(store_a, store_f):
        def cb(i, alpha, u8, out):
            store_a[i] = out[3][0, 0, 0].clone()
            store_f[i] = core._engine.last_fgr.clone()
        return cb
    got = run_video_matte(m, frames, trimap=tri, keyframes={2: lab}, foreground=True, new_background=bg, work_scale=s,
                          work_radius=r, work_eps=eps, on_frame=grab(work_alpha, work_fgr), **kw)
    assert core.foreground is False
    # the network's own run on the restatement-reduced inputs (same process: the tuner's choices are shared)
    frames_w = [R.downsample_u8(f, s) for f in frames]
    tri_w, lab_w = R.downsample_trimap(tri, s), R.downsample_labels(lab, s)
    d_alpha, d_fgr = {}, {}
    direct = run_video_matte(m, frames_w, trimap=tri_w, keyframes={2: lab_w}, foreground=True, on_frame=grab(d_alpha, d_fgr), **kw)
    h, w = R.work_size(H, W, s)
    assert got["work_size"] == (h, w) == (48, 64)
    assert tuple(got["alpha"].shape) == (T, H, W) and tuple(got["alpha_u8"].shape) == (T, H, W)
    assert tuple(got["fgr_u8"].shape) == (T, H, W, 4) and tuple(got["comp_u8"].shape) == (T, H, W, 3)
    assert tuple(got["trimap"].shape) == (T, 3, h, w)
    assert torch.equal(got["trimap"], direct["trimap"])
    assert got["bank_frames"] == direct["bank_frames"] and got["schedule"] == direct["schedule"]
    for t in range(T):
        assert torch.equal(work_alpha[t], direct["alpha"][t].to(work_alpha[t].device)), t
        assert torch.equal(work_alpha[t], d_alpha[t]) and torch.equal(work_fgr[t], d_fgr[t]), t
        tg = [work_alpha[t].cpu().numpy()] + list(work_fgr[t].cpu().numpy())
        a, u8, F = R.guided_upsample(frames[t], frames_w[t], tg, s, r, eps)
        _, rgba, comp = fgr_ref.fgr_outputs(a, F, bg=bg, u8_rgb=False)
        assert np.array_equal(bits(got["alpha"][t].numpy()), bits(a)), t
        assert np.array_equal(got["alpha_u8"][t].numpy(), u8), t
        assert np.array_equal(got["fgr_u8"][t].numpy(), rgba), t
        assert np.array_equal(got["comp_u8"][t].numpy(), comp), t
    assert "work_size" not in before and sorted(before) == ["alpha", "alpha_u8", "anchor_frames", "bank_frames", "schedule", "trimap"]
    after = run_video_matte(m, frames, trimap=tri, keyframes={2: lab}, **kw)
    for k in ("alpha", "alpha_u8", "trimap"):
        assert torch.equal(after[k], before[k]), k
    assert after["bank_frames"] == before["bank_frames"]
    # alpha alone (one target), and a colour background
    a_only = run_video_matte(m, frames, trimap=tri, keyframes={2: lab}, work_scale=s, work_radius=r, work_eps=eps, **kw)
    assert sorted(a_only) == ["alpha", "alpha_u8", "anchor_frames", "bank_frames", "schedule", "trimap", "work_size"]
    assert torch.equal(a_only["alpha"], got["alpha"]) and torch.equal(a_only["alpha_u8"], got["alpha_u8"])
    # on_foreground: the same bytes handed over per frame instead of collected
    seen = {}
    handed = run_video_matte(m, frames, trimap=tri, keyframes={2: lab}, foreground=True, new_background=bg, work_scale=s,
                             work_radius=r, work_eps=eps, on_foreground=lambda i, f, c: seen.__setitem__(i, (f.cpu(), c.cpu())), **kw)
    assert "fgr_u8" not in handed and "comp_u8" not in handed and sorted(seen) == list(range(T))
    for t in range(T):
        assert torch.equal(seen[t][0], got["fgr_u8"][t]) and torch.equal(seen[t][1], got["comp_u8"][t])


def test_eval_cli_work_scale_writes_full_resolution_pngs(G, tmp_path, synth_sd):
    import json
    from PIL import Image
    from tests.test_gpu_frame import _fresh_model
    from otvm_amd import eval_cli
    from otvm_amd.datasets import Demo_Test, load_sequence
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.video import run_video_matte
    H, W, T = 64, 96, 3
    frames_bgr, tri = synthetic_clip(H, W, T, 41)
    demo = os.path.join(str(tmp_path), "demo")
    os.makedirs(os.path.join(demo, "clip", "frames")); os.makedirs(os.path.join(demo, "clip", "trimap"))
    for t in range(T):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
    Image.fromarray((np.asarray(tri)[1] * 128 + np.asarray(tri)[2] * 255).astype(np.uint8)).save(
        os.path.join(demo, "clip", "trimap", "0000.png"))
    out = os.path.join(str(tmp_path), "out")
    sj = os.path.join(str(tmp_path), "summary.json")
    res = eval_cli.main(["--demo", "--data", demo, "--synthetic-weights", "--skip", "2", "--out", out, "--work-scale", "2", "--fgr",
                         "--composite", "10,200,30", "--summary-json", sj])
    assert res["frames"] == T
    summary = json.load(open(sj))
    assert summary["work_scale"] == 2 and summary["work_size"] == {"clip": [32, 48]}
    m = _fresh_model(synth_sd, 12, "f16x3")
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames_bgr]
    d = load_sequence(next(iter(Demo_Test(demo))))
    ref = run_video_matte(m, rgb, trimap=d["trimap"], skip=2, max_num=5, frames_are_rgb=True, foreground=True,
                          new_background=(10, 200, 30), work_scale=2)
    for t in range(T):
        n = "%04d.png" % t
        a = np.asarray(Image.open(os.path.join(out, "alpha", "test", "s4_OTVM", "pred", "clip", n)))
        f = Image.open(os.path.join(out, "fgr", "clip", n))
        c = Image.open(os.path.join(out, "comp", "clip", n))
        assert a.shape == (H, W) and f.size == (W, H) and c.size == (W, H) and f.mode == "RGBA" and c.mode == "RGB"
        assert np.array_equal(a, ref["alpha_u8"][t].numpy())
        assert np.array_equal(np.asarray(f), ref["fgr_u8"][t].numpy())
        assert np.array_equal(np.asarray(c), ref["comp_u8"][t].numpy())
    with pytest.raises(SystemExit):
        eval_cli.main(["--demo", "--data", demo, "--synthetic-weights", "--out", out, "--work-scale", "2", "--viz"])
