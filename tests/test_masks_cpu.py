"""CPU: trimaps from masks -- the capped separable restatement against the brute-force definition (tests/mask_trimap_ref.py), a
disc's band, the Mask value object and the argument rules of run_video_matte / eval_cli that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mask_trimap_cases as K
from tests import mask_trimap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("H,W", K.CPU_SIZES, ids=["%dx%d" % s for s in K.CPU_SIZES])
def test_capped_restatement_equals_brute_force(H, W):
    masks = [("soft", K.soft_mask(H, W, 3 * H + W))]
    masks += [("p%g" % p, K.density_mask(H, W, p, H + W)) for p in (0.0, 0.03, 0.5, 0.97, 1.0)]       # empty ... full
    masks += [("one-fg", K.one_pixel(H, W, 255)), ("one-bg", K.one_pixel(H, W, 0))]
    for name, m in masks:
        for lo, hi in K.THRESHOLDS:
            for t in K.CPU_T_VALUES:
                t_bg = K.CPU_T_VALUES[(K.CPU_T_VALUES.index(t) + 2) % len(K.CPU_T_VALUES)]            # the two sets differ
                a, b = R.classes(m, lo, hi, t, t_bg), R.classes(m, lo, hi, t, t_bg, brute=True)
                assert np.array_equal(a, b), (name, lo, hi, t, t_bg)
    full = np.full((H, W), 255, np.uint8)
    assert (R.classes(full, 127, 128, 400, 400) == 2).all()          # no pixel outside the set: d = +inf, the edge seeds nothing
    assert (R.classes(np.zeros((H, W), np.uint8), 127, 128, 400, 400) == 0).all()


def test_radius_zero_is_the_thresholded_mask():
    m = K.soft_mask(33, 47, 5)
    for lo, hi in K.THRESHOLDS:
        cls = R.classes(m, lo, hi, R.band_t(0), R.band_t(0))
        assert np.array_equal(cls == 2, m >= hi) and np.array_equal(cls == 0, m <= lo)
        assert np.array_equal(cls == 1, (m > lo) & (m < hi))


def test_disc_mask_band():
    H, W, cy, cx, rad, r = 90, 100, 44, 52, 30, 5
    m = K.disc(H, W, cy, cx, rad)
    cls = R.classes(m, 127, 128, R.band_t(r), R.band_t(r))
    assert (m[cls == 2] == 255).all() and (cls == 2).sum() > 0            # fg inside the disc
    assert (m[cls == 0] == 0).all() and (cls == 0).sum() > 0              # bg outside it
    yy, xx = np.mgrid[0:H, 0:W]
    to_boundary = np.abs(np.sqrt(((yy - cy) ** 2 + (xx - cx) ** 2).astype(np.float64)) - rad)
    assert (cls[to_boundary < 4] == 1).all()
    assert (cls[to_boundary > 7] != 1).all()                             # and the band is a band
    # a subject cut by the frame edge stays foreground up to the edge
    cut = K.disc(60, 60, 0, 30, 25)
    c2 = R.classes(cut, 127, 128, R.band_t(5), R.band_t(5))
    assert (c2[0, 12:49] == 2).all()


def test_quantise_and_band_t():
    from otvm_amd import masks
    x = np.array([[-0.5, 0.0, 0.001, 0.4999], [0.5, 0.998, 1.0, 7.0]], np.float32)
    want = R.quantise(x)
    assert want.tolist() == [[0, 0, 0, 127], [128, 254, 255, 255]]
    assert np.array_equal(masks.quantise(torch.from_numpy(x)).numpy(), want)
    u = torch.arange(6, dtype=torch.uint8).view(2, 3)
    assert masks.quantise(u) is u
    for r in (0, 1, 1.5, 2.9, 5, 12, 20, 255, 254.999):
        assert masks.band_thresholds(r) == (R.band_t(r), R.band_t(r))
    assert masks.band_thresholds((5, 12.5)) == (25, 156) and masks.band_thresholds(255) == (65025, 65025)
    for bad in (-1, 255.5, 256, "5", None, (1, 2, 3), (1, -2), True):
        with pytest.raises(ValueError):
            masks.band_thresholds(bad)


def test_mask_validation():
    from otvm_amd.masks import Mask, as_mask
    m = np.zeros((4, 6), np.uint8)
    k = Mask(m)
    assert (k.role, k.band, k.lo, k.hi, k.shape) == ("key", None, 127, 128, (4, 6))
    assert Mask(torch.zeros(4, 6), band=(3, 4.5), lo=0, hi=255, role="labels").role == "labels"
    assert as_mask(k, "x") is k and as_mask(m, "x").shape == (4, 6)
    with pytest.raises(ValueError, match="role"):
        Mask(m, role="correction")
    with pytest.raises(ValueError, match="lo >= hi"):
        Mask(m, lo=128, hi=128)
    with pytest.raises(ValueError, match="lo >= hi"):
        Mask(m, lo=200, hi=100)
    with pytest.raises(ValueError):
        Mask(m, lo=-1, hi=5)
    with pytest.raises(ValueError):
        Mask(m, hi=256)
    with pytest.raises(ValueError, match="0 ... 255"):
        Mask(m, band=256)
    with pytest.raises(ValueError, match="0 ... 255"):
        Mask(m, band=(5, -1))
    with pytest.raises(ValueError, match="one plane"):
        Mask(np.zeros((3, 4, 6), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        Mask(np.zeros((4, 6), np.int32))
    with pytest.raises(ValueError, match="x: Mask"):
        as_mask(np.zeros((4, 6, 3), np.uint8), "x")

    class WithKernel:
        DILATION_KERNEL = 12

    class Without:
        pass

    class Wrapped:
        module = WithKernel()
    assert k.band_for(WithKernel()) == 12 and k.band_for(Wrapped()) == 12 and Mask(m, band=3).band_for(Without()) == 3
    with pytest.raises(ValueError, match="band"):
        k.band_for(Without())


def test_keyframe_kind_and_schedule_learn_mask():
    from otvm_amd.masks import Mask
    from otvm_amd.video import _keyframe_kind, keyframe_schedule
    m = np.zeros((4, 6), np.uint8)
    assert _keyframe_kind(Mask(m)) == "key" and _keyframe_kind(Mask(m, role="labels")) == "labels"
    assert _keyframe_kind(m) == "labels" and _keyframe_kind(np.zeros((3, 4, 6), np.float32)) == "key"
    assert keyframe_schedule(5, {0: Mask(m), 3: Mask(m), 4: Mask(m, role="labels")}, 10) == keyframe_schedule(
        5, {0: "key", 3: "key", 4: "labels"}, 10)


class _NoDevice(torch.nn.Module):
    """Stands where the model does: the argument rules are checked before any device work."""
    DILATION_KERNEL = 12

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_run_video_matte_exclusivity_rules():
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    model = _NoDevice()
    H, W, T = 6, 8, 3
    frames = [np.zeros((H, W, 3), np.uint8)] * T
    m = np.zeros((H, W), np.uint8)
    tri = np.zeros((3, H, W), np.float32)
    ms = [m] * T
    for kw, word in ((dict(masks=ms, trimap=tri), "trimap"), (dict(masks=ms, mask=m), "mask"),
                     (dict(masks=ms, keyframes={1: tri}), "keyframes"), (dict(masks=ms, alphas=[m] * T), "alphas"),
                     (dict(masks=ms[:2]), "one mask per frame"),
                     (dict(masks=[m, Mask(m, role="labels"), m]), "role"),
                     (dict(mask=Mask(m, role="labels")), "role"),
                     (dict(mask=m, trimap=tri), "both"), (dict(mask=m, keyframes={0: tri}), "both"),
                     (dict(mask=m, alphas=[m] * T), "alphas"),
                     (dict(masks=[m, np.zeros((3, H, W), np.uint8), m]), "one plane")):
        with pytest.raises(ValueError, match=word):
            run_video_matte(model, frames, **kw)
    model.DILATION_KERNEL = None
    with pytest.raises(ValueError, match="band"):
        run_video_matte(model, frames, masks=ms)
    for kw in (dict(mask=m), dict(masks=[ms]), dict(trimaps=[Mask(m)])):
        with pytest.raises(ValueError, match="single-clip"):
            run_video_matte_batch(model, [frames], **({"trimaps": [tri]} | kw))


def test_eval_cli_refuses_masks_outside_their_route(tmp_path):
    from otvm_amd import eval_cli
    data = str(tmp_path)
    for argv, word in ((["--masks", "key"], "--demo"), (["--demo", "--masks", "frame", "--batch", "2"], "--batch"),
                       (["--demo", "--masks", "frame", "--keyframes"], "--keyframes"),
                       (["--demo", "--masks", "key", "--mask-band", "300"], "--mask-band"),
                       (["--demo", "--masks", "key", "--mask-band", "1,2,3"], "--mask-band"),
                       (["--demo", "--masks", "key", "--mask-thresholds", "128,128"], "--mask-thresholds"),
                       (["--demo", "--masks", "key", "--mask-thresholds", "5"], "--mask-thresholds")):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(["--data", data, "--synthetic-weights"] + argv)
        assert word in str(e.value), (argv, str(e.value))
    assert eval_cli.parse_mask_options("5,12.5", "25,230") == ((5.0, 12.5), (25, 230))
    assert eval_cli.parse_mask_options(None, "127,128") == (None, (127, 128))


def test_load_sequence_reads_mask_files(tmp_path):
    from PIL import Image
    from otvm_amd.datasets import Demo_Test, load_sequence
    root = os.path.join(str(tmp_path), "demo")
    for sub in ("frames", "mask"):
        os.makedirs(os.path.join(root, "clip", sub))
    g = np.random.default_rng(1)
    for t in range(3):
        Image.fromarray(g.integers(0, 256, (5, 7, 3), dtype=np.uint8)).save(os.path.join(root, "clip", "frames", "%04d.png" % t))
    m = g.integers(0, 256, (5, 7), dtype=np.uint8)
    Image.fromarray(m).save(os.path.join(root, "clip", "mask", "0001.png"))
    item = next(iter(Demo_Test(root)))
    with pytest.raises(FileNotFoundError):
        load_sequence(item)                                  # as before: no trimap for the first frame
    d = load_sequence(item, masks=True)
    assert d["trimap"] is None and sorted(d["mask_maps"]) == [1] and np.array_equal(d["mask_maps"][1], m)
    d = load_sequence(item, keyframes=True, masks=True)
    assert d["keyframe_trimaps"] == {} and d["label_maps"] == {} and sorted(d["mask_maps"]) == [1]


def test_binding_declares_the_mask_entry_points():
    import __graft_entry__ as g
    from otvm_amd import lib as L
    h = ctypes.CDLL(g.build())
    for sym in ("otvm_trimap_from_mask", "otvm_trimap_from_mask_ws_bytes"):
        assert sym in L.EXPORTED and getattr(h, sym) is not None
    h.otvm_trimap_from_mask_ws_bytes.restype = ctypes.c_int64
    assert h.otvm_trimap_from_mask_ws_bytes(1080, 1920) == 1080 * 1920 * 2
    for bad in ((0, 5), (5, 0), (16384, 5), (5, 16384), (-3, 4)):
        assert h.otvm_trimap_from_mask_ws_bytes(*bad) == -1
    assert h.otvm_trimap_from_mask_ws_bytes(16383, 16383) == 16383 * 16383 * 2
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    # the C struct and the ctypes struct name the same fields in the same order
    body = header[header.index("typedef struct otvm_mask_trimap_params {"):header.index("} otvm_mask_trimap_params;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^(const\s+)?\w+\*?\s+", "", decl.strip()).split(",")]
    assert names == [f for f, _ in L.MaskTrimapParams._fields_], names
    assert ctypes.sizeof(L.MaskTrimapParams) == 56
