"""GPU (-m gpu): trimap-free matting of keyed footage -- otvm_mask_from_chroma and otvm_mask_from_plate bit for bit against their
restatement (tests/key_ref.py: held to the float64 definition in tests/test_key_cpu.py), and run_video_matte(key=...), eval_cli
--key and y4m_cli --key BY DEFINITION: the same bytes as the ``masks=`` route fed the restatement's masks."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import key_ref as K
from tests import mask_trimap_ref as MR
from tests import yuv_ref as Y

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SENT, PAD = 0xA5, 64
GREEN, BLUE, TEAL = (0, 255, 0), (0, 0, 255), (20, 170, 150)
SIZES = [(1, 1), (1, 37), (37, 1), (33, 70), (135, 241), (64, 96)]          # (H, W); 64 x 96 takes the dword path


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from otvm_amd import lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _buffers(arrays, H, W, off):
    """Every input [H,W,3] in a buffer of its own at byte offset ``off``; the mask in a buffer of sentinels, PAD + off bytes in"""
    ins = []
    for a in arrays:
        buf = torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device=DEV)
        buf[off:off + H * W * 3] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)
        ins.append(buf)
    out = torch.full((H * W + 2 * PAD + 8,), SENT, dtype=torch.uint8, device=DEV)
    return ins, out


def _mask_of(out, H, W, off):
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    a = PAD + off
    assert (o[:a] == SENT).all() and (o[a + H * W:] == SENT).all(), "bytes round the mask were written"
    return o[a:a + H * W].reshape(H, W).copy()


def raw_chroma(lib, frame, kb, kr, qlo, qhi, rgb, off=0, rc=0):
    from otvm_amd import lib as L
    H, W = frame.shape[:2]
    (f,), out = _buffers([frame], H, W, off)
    p = L.MaskFromChromaParams(frame=f.data_ptr() + off, mask=out.data_ptr() + PAD + off, H=H, W=W, u8_rgb=int(rgb), kb=kb, kr=kr,
                               qlo=qlo, qhi=qhi)
    got = lib.otvm_mask_from_chroma(C.byref(p), _stream())
    assert (got != 0) == (rc != 0), lib.otvm_last_error().decode()
    return _mask_of(out, H, W, off)


def raw_plate(lib, frame, plate, radius, lo, hi, off=0, rc=0):
    from otvm_amd import lib as L
    H, W = frame.shape[:2]
    (f, pl), out = _buffers([frame, plate], H, W, off)
    p = L.MaskFromPlateParams(frame=f.data_ptr() + off, plate=pl.data_ptr() + off, mask=out.data_ptr() + PAD + off, H=H, W=W,
                              radius=radius, lo=lo, hi=hi)
    got = lib.otvm_mask_from_plate(C.byref(p), _stream())
    assert (got != 0) == (rc != 0), lib.otvm_last_error().decode()
    return _mask_of(out, H, W, off)


def _random(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _near_key(H, W, colour, seed):
    """Pixels scattered round the key colour at every brightness: their q spreads over both thresholds"""
    g = np.random.default_rng(seed)
    s = g.random((H, W, 1))
    px = np.asarray(colour, np.float64)[None, None] * s + g.normal(0, 25, (H, W, 3)) + 40 * (1 - s)
    return np.clip(np.round(px), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ otvm_mask_from_chroma
@pytest.mark.parametrize("H,W", SIZES)
def test_chroma_key_equals_the_restatement(lib, H, W):
    seen = set()
    for colour, (lo, hi) in ((GREEN, (8, 24)), (BLUE, (8, 8.008)), (TEAL, (-5, 60))):
        kb, kr = K.key_chroma(colour)
        qlo, qhi = K.thresholds(kb, kr, lo, hi)
        if colour == BLUE:
            assert qhi == qlo + 1                                       # the narrowest ramp there is
        for rgb in (True, False):
            for frame in (_random(H, W, H * W + rgb), _near_key(H, W, colour if rgb else colour[::-1], 3 * H + W)):
                want = K.mask_from_chroma(frame, kb, kr, qlo, qhi, rgb=rgb)
                assert np.array_equal(raw_chroma(lib, frame, kb, kr, qlo, qhi, rgb), want), (colour, rgb)
                seen |= set(np.unique(want).tolist())
    if H * W > 1000:
        assert {0, 255} <= seen and len(seen) > 20                      # the ramp was exercised, not only its ends


@pytest.mark.parametrize("H,W", [(33, 70), (64, 96)])
def test_chroma_key_pixels_placed_on_the_thresholds(lib, H, W):
    """qlo and qhi are taken from the q the restatement gives pixels of the image itself: pixels sit exactly ON both thresholds
    and one step inside them."""
    kb, kr = K.key_chroma(GREEN)
    frame = _near_key(H, W, GREEN, 5)
    q = np.unique(K.chroma_q(frame, kb, kr, rgb=True))
    inside = q[(q > 500) & (q < 6000)]
    assert inside.size > 50
    for qlo, qhi in ((int(inside[3]), int(inside[-3])), (int(inside[20]), int(inside[21])), (int(inside[10]), int(inside[10]) + 1)):
        want = K.mask_from_chroma(frame, kb, kr, qlo, qhi, rgb=True)
        qq = K.chroma_q(frame, kb, kr, rgb=True)
        assert (qq == qlo).any() and ((qq == qhi).any() or qhi == qlo + 1)      # (the narrowest ramp: a pixel on qlo is enough)
        assert (want[qq == qlo] == 255).all() and (want[qq == qhi] == 0).all()
        assert np.array_equal(raw_chroma(lib, frame, kb, kr, qlo, qhi, True), want)


# ------------------------------------------------------------------------------------------------ otvm_mask_from_plate
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_plate_key_equals_the_restatement(lib, H, W, radius):
    g = np.random.default_rng(H + 7 * W + radius)
    plate = _random(H, W, 11 * H + W)
    near = np.clip(plate.astype(int) + g.integers(-60, 61, plate.shape), 0, 255).astype(np.uint8)
    border = plate.copy()                                               # differs from the plate in the outermost row and column only:
    other = _random(H, W, 5)                                            # the border clamp and the halo decide its mask
    border[0], border[-1], border[:, 0], border[:, -1] = other[0], other[-1], other[:, 0], other[:, -1]
    for lo, hi in ((12, 40), (20, 21), (0, 255)):
        for frame in (_random(H, W, 3 * H + W), near, border):
            want = K.mask_from_plate(frame, plate, radius, lo, hi)
            assert np.array_equal(raw_plate(lib, frame, plate, radius, lo, hi), want), (lo, hi)
    if H > 2 and W > 2:
        m = K.mask_from_plate(border, plate, radius, 12, 40)
        assert (m[1:-1, 1:-1] == 0).all() and (m != 0).any()


@pytest.mark.parametrize("H,W", [(33, 70), (64, 96)])
def test_plate_key_pixels_placed_on_the_thresholds(lib, H, W):
    """A uniform plate, so that the neighbourhood changes nothing: d is the frame's own offset, which runs through 0 ... 255 --
    pixels sit exactly on lo, lo + 1, hi - 1 and hi."""
    plate = np.full((H, W, 3), 0, np.uint8)
    d = (np.arange(H * W) % 256).reshape(H, W).astype(np.uint8)
    frame = np.stack([d, d // 2, d // 3], -1)
    for radius in (0, 3):
        for lo, hi in ((12, 40), (99, 100), (0, 1), (254, 255)):
            want = K.mask_from_plate(frame, plate, radius, lo, hi)
            assert (want[d == lo] == 0).all() and (want[d == hi] == 255).all() and (d == lo).any() and (d == hi).any()
            assert np.array_equal(raw_plate(lib, frame, plate, radius, lo, hi), want)


# ------------------------------------------------------------------------------------------------ both
def test_an_unaligned_base_takes_the_scalar_path_with_equal_bits(lib):
    H, W = 64, 96
    frame, plate = _near_key(H, W, GREEN, 9), _random(H, W, 10)
    kb, kr = K.key_chroma(GREEN)
    qlo, qhi = K.thresholds(kb, kr, 8, 24)
    a = raw_chroma(lib, frame, kb, kr, qlo, qhi, True, off=0)
    b = raw_chroma(lib, frame, kb, kr, qlo, qhi, True, off=1)
    assert np.array_equal(a, b) and np.array_equal(a, K.mask_from_chroma(frame, kb, kr, qlo, qhi, rgb=True))
    near = np.clip(plate.astype(int) + np.random.default_rng(1).integers(-60, 61, plate.shape), 0, 255).astype(np.uint8)
    a = raw_plate(lib, near, plate, 2, 12, 40, off=0)
    b = raw_plate(lib, near, plate, 2, 12, 40, off=1)
    assert np.array_equal(a, b) and np.array_equal(a, K.mask_from_plate(near, plate, 2, 12, 40))


def test_1080p_every_element_twice_and_the_wrapper(lib):
    from otvm_amd import keys
    H, W = 1080, 1920
    frame = _near_key(H, W, GREEN, 21)
    kb, kr = K.key_chroma(GREEN)
    qlo, qhi = K.thresholds(kb, kr, 8, 24)
    want = K.mask_from_chroma(frame, kb, kr, qlo, qhi, rgb=False)
    a, b = (raw_chroma(lib, frame, kb, kr, qlo, qhi, False) for _ in range(2))
    assert np.array_equal(a, want) and np.array_equal(a, b)
    fd = torch.from_numpy(frame).to(DEV)
    assert np.array_equal(keys.key_mask(fd, keys.ChromaKey("green")).cpu().numpy(), want)
    assert np.array_equal(keys.key_mask(fd, keys.ChromaKey("green"), rgb=True).cpu().numpy(),
                          K.mask_from_chroma(frame, kb, kr, qlo, qhi, rgb=True))
    plate = _random(H // 8, W // 8, 22).repeat(8, 0).repeat(8, 1)       # blocks: the neighbourhood finds closer pixels across their edges
    near = np.clip(plate.astype(int) + np.random.default_rng(23).integers(-50, 51, plate.shape), 0, 255).astype(np.uint8)
    near[200:600, 300:900] = _random(400, 600, 24)
    want = K.mask_from_plate(near, plate, 2, 12, 40)
    a, b = (raw_plate(lib, near, plate, 2, 12, 40) for _ in range(2))
    assert np.array_equal(a, want) and np.array_equal(a, b)
    got = keys.key_mask(torch.from_numpy(near).to(DEV), keys.PlateKey(plate, radius=2))
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="plate"):
        keys.key_mask(fd[:100], keys.PlateKey(plate))


def test_bad_arguments_launch_nothing(lib):
    frame = _random(8, 12, 1)
    kb, kr = K.key_chroma(GREEN)
    for bad in (dict(kb=3, kr=-15), dict(qlo=300, qhi=300), dict(qlo=301, qhi=300)):
        args = dict(kb=kb, kr=kr, qlo=100, qhi=300)
        args.update(bad)
        m = raw_chroma(lib, frame, args["kb"], args["kr"], args["qlo"], args["qhi"], True, rc=1)
        assert (m == SENT).all() and lib.otvm_last_error().decode().startswith("otvm_mask_from_chroma")
    for radius, lo, hi in ((4, 12, 40), (-1, 12, 40), (1, 40, 12), (1, 12, 12), (1, 0, 256)):
        m = raw_plate(lib, frame, frame, radius, lo, hi, rc=1)
        assert (m == SENT).all() and lib.otvm_last_error().decode().startswith("otvm_mask_from_plate")


# ------------------------------------------------------------------------------------------------ the route, by definition
H_, W_, T_ = 160, 224, 6
FIELD, DISC = (30, 200, 40), (200, 60, 90)                               # R, G, B
KEY_KW = dict(lo=8, hi=24)
PLATE_KW = dict(lo=12, hi=40, radius=1)
RUN = dict(skip=2, max_num=3)
WINDOW = (16, 16, 128, 192)


def _clip():
    """A noisy green field with a moving soft-edged disc of a colour that is not green, B, G, R as decoded frames are; the clean
    plate: the field without the disc, with FRESH noise (frame and plate differ by at most 8 <= lo off the disc)."""
    g = np.random.default_rng(71)
    yy, xx = np.mgrid[0:H_, 0:W_]
    field, disc = np.asarray(FIELD, np.float64), np.asarray(DISC, np.float64)
    frames = []
    for t in range(T_):
        r = np.sqrt((yy - (H_ / 2 + 2 * t)) ** 2 + (xx - (W_ / 2 - 20 + 8 * t)) ** 2)
        a = np.clip((38 - r) / 6.0 + 0.5, 0, 1)[..., None]
        rgb = field * (1 - a) + disc * a + g.integers(-4, 5, (H_, W_, 3))
        frames.append(np.ascontiguousarray(np.clip(np.round(rgb), 0, 255).astype(np.uint8)[..., ::-1]))
    plate = np.clip(field[None, None] + g.integers(-4, 5, (H_, W_, 3)), 0, 255).astype(np.uint8)[..., ::-1]
    return frames, np.ascontiguousarray(plate)


@pytest.fixture(scope="module")
def route(lib, synth_sd, tmp_path_factory):
    """One model for all route tests, with the kernel configurations fixed and shared through a file (the command lines' own
    models launch the same ones); the clip, its plate, and the restatement's masks of both keys -- computed once."""
    from otvm_amd import engine
    from tests.test_gpu_frame import _fresh_model
    old, old_auto = os.environ.get("OTVM_TUNE_FILE"), engine.AUTOTUNE
    os.environ["OTVM_TUNE_FILE"] = os.path.join(str(tmp_path_factory.mktemp("tune")), "tune.json")
    engine.AUTOTUNE = False
    try:
        frames, plate = _clip()
        chroma = [K.chroma_key_mask(f, GREEN, **KEY_KW, rgb=False) for f in frames]
        plated = [K.mask_from_plate(f, plate, PLATE_KW["radius"], PLATE_KW["lo"], PLATE_KW["hi"]) for f in frames]
        for ms in (chroma, plated):
            for m in ms:                                                 # all three classes on every frame (band: the model's 12)
                tri = MR.trimap_from_mask(m, 12)
                assert all(tri[c].any() for c in range(3))
                assert 0 < (m > 0).mean() < 0.5 and ((m > 0) & (m < 255)).any()
        yield _fresh_model(synth_sd, 12, "f16x3"), frames, plate, chroma, plated
    finally:
        engine.AUTOTUNE = old_auto
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


def _same(a, b, keys=("alpha", "alpha_u8", "trimap")):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k
    assert a["bank_frames"] == b["bank_frames"] == [[]] * len(a["bank_frames"])


class _OneShot:
    """A source that hands every frame out once, in order, from an iterator (a pipe)"""

    def __init__(self, frames):
        self.it, self.n, self.i = iter(frames), len(frames), 0

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        assert i == self.i, "frame %d asked for, frame %d is next: a second read" % (i, self.i)
        self.i += 1
        return next(self.it)


CASES = {"plain": {}, "work_scale": dict(work_scale=2), "stabilise": dict(stabilise=True),
         "foreground": dict(foreground=True, new_background=(10, 200, 30)), "window": dict(roi=WINDOW), "auto": dict(roi="auto", roi_margin=8)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("which", ["chroma", "plate"])
def test_key_route_equals_the_masks_route_on_the_restated_masks(route, which, case):
    from otvm_amd import keys
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    key = keys.ChromaKey("green", **KEY_KW) if which == "chroma" else keys.PlateKey(plate, **PLATE_KW)
    masks = chroma if which == "chroma" else plated
    kw = dict(RUN, **CASES[case])
    got = run_video_matte(m, frames, key=key, **kw)
    want = run_video_matte(m, frames, masks=[Mask(x) for x in masks], **kw)
    extra = {"stabilise": ("alpha_raw",), "foreground": ("fgr_u8", "comp_u8")}.get(case, ())
    _same(got, want, ("alpha", "alpha_u8", "trimap") + extra)
    assert sorted(got) == sorted(want)
    if case == "work_scale":
        assert got["work_size"] == want["work_size"] == (80, 112)
    if case in ("window", "auto"):
        assert (got["roi"], got["roi_size"], got["roi_clipped"]) == (want["roi"], want["roi_size"], want["roi_clipped"])
        assert len(set(got["roi"])) > 1 if case == "auto" else got["roi"] == [WINDOW] * T_


def test_key_route_from_a_source_that_is_read_once(route):
    from otvm_amd import keys
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames]
    key = keys.ChromaKey("green", **KEY_KW)
    src = _OneShot(rgb)
    got = run_video_matte(m, src, key=key, frames_are_rgb=True, **RUN)
    assert src.i == T_
    _same(got, run_video_matte(m, rgb, masks=[Mask(x) for x in chroma], frames_are_rgb=True, **RUN))
    src = _OneShot(rgb)
    _same(run_video_matte(m, src, key=key, frames_are_rgb=True, roi=WINDOW, **RUN),
          run_video_matte(m, rgb, masks=[Mask(x) for x in chroma], frames_are_rgb=True, roi=WINDOW, **RUN))
    src = _OneShot(rgb)
    with pytest.raises(ValueError, match="roi='auto'.*window"):
        run_video_matte(m, src, key=key, frames_are_rgb=True, roi="auto", **RUN)
    assert src.i == 0
    with pytest.raises(ValueError, match="plate of `key`"):               # a streaming source: refused at the first frame
        run_video_matte(m, _OneShot(rgb), key=keys.PlateKey(plate[:100]), frames_are_rgb=True, **RUN)


def test_the_key_adds_no_read_back_to_the_frame_loop(route, monkeypatch):
    """Every way a tensor reaches the host is counted -- .cpu(), .item(), .tolist(), .numpy(), bool / int / float of a device tensor,
    .to() that lands on the host, copy_() from the device into a host tensor -- and so is torch.cuda.synchronize.  The ONLY ones the
    frame loop may make are the engine's own, named here: HipEngine.guard_check and HipEngine.predict_check, which read a flag
    and the conditioning words on the first frame of a clip (every frame of this route is one) -- events "engine".  Everything
    else must be absent: no copy inside the key's own work (the launch and the mask-to-trimap step, KeyedMask.convert), none
    anywhere else in the loop, no synchronisation; roi="auto" adds exactly one read-back, of T boxes, before the first frame.
    The list also equals, entry for entry, that of the ``masks=`` route with its masks resident on the device."""
    from otvm_amd import engine, keys, roi
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    events, state = [], {"in_convert": 0, "quiet": 0, "engine": 0}

    def note():
        if not state["quiet"]:
            events.append("engine" if state["engine"] else "copy-in-convert" if state["in_convert"] else "copy")

    def counting(name, reaches_host):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            quiet = state["quiet"]
            state["quiet"] += 1
            try:
                out = real(self, *a, **k)
            finally:
                state["quiet"] -= 1
            if not quiet and reaches_host(self, a, out):
                note()
            return out
        return f
    from_device = lambda self, a, out: self.is_cuda
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, counting(name, from_device))
    monkeypatch.setattr(torch.Tensor, "to", counting("to", lambda self, a, out: self.is_cuda and not out.is_cuda))
    monkeypatch.setattr(torch.Tensor, "copy_", counting("copy_", lambda self, a, out: not self.is_cuda and len(a) > 0 and a[0].is_cuda))
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (events.append("sync"), real_sync(*a, **k))[1])

    def inside(flag, real):
        def f(*a, **k):
            state[flag] += 1
            try:
                return real(*a, **k)
            finally:
                state[flag] -= 1
        return f
    monkeypatch.setattr(keys.KeyedMask, "convert", inside("in_convert", keys.KeyedMask.convert))
    monkeypatch.setattr(engine.HipEngine, "guard_check", inside("engine", engine.HipEngine.guard_check))
    monkeypatch.setattr(engine.HipEngine, "predict_check", inside("engine", engine.HipEngine.predict_check))
    real_boxes = roi.boxes_of

    def boxes(rows):
        events.append("boxes")
        state["quiet"] += 1
        try:
            return real_boxes(rows)
        finally:
            state["quiet"] -= 1
    monkeypatch.setattr(roi, "boxes_of", boxes)
    on_dev = [Mask(torch.from_numpy(x).to(DEV)) for x in chroma]
    for kw in ({}, dict(roi="auto"), dict(work_scale=2)):
        run_video_matte(m, frames, masks=on_dev, keep_on_device=True, **RUN, **kw)    # (the engine's plan for this size exists from here on)
        del events[:]
        run_video_matte(m, frames, key=keys.ChromaKey("green", **KEY_KW), keep_on_device=True,
                        on_frame=lambda i, a, u8, out: events.append(i), **RUN, **kw)
        keyed = list(events)
        del events[:]
        run_video_matte(m, frames, masks=on_dev, keep_on_device=True, on_frame=lambda i, a, u8, out: events.append(i), **RUN, **kw)
        print("read-backs of the clip", kw, keyed)
        # the baseline, named: frame indices in order, the engine's own first-frame checks, roi="auto"'s one read-back -- nothing else
        assert set(keyed) <= set(range(T_)) | {"engine"} | ({"boxes"} if "roi" in kw else set()), keyed
        assert [e for e in keyed if isinstance(e, int)] == list(range(T_))
        assert [e for e in keyed if e == "boxes"] == (["boxes"] if "roi" in kw else [])
        if "roi" in kw:
            assert keyed[0] == "boxes"                                             # the one read-back: before anything else
        assert keyed == events, kw


def test_a_window_is_held_against_every_band_where_the_source_can_be_read_twice(route):
    """As ``masks=`` does: a window that does not hold a frame's unknown band is refused, by the same pre-pass, with the same
    message.  A source that is read once allows no pre-pass: the window is taken as it is (and, where it does hold the bands,
    gives the same bytes: test_key_route_from_a_source_that_is_read_once)."""
    from otvm_amd import keys
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    small = (32, 32, 96, 128)                                                      # the disc's band leaves it on every frame
    key = keys.ChromaKey("green", **KEY_KW)
    with pytest.raises(ValueError) as want:
        run_video_matte(m, frames, masks=[Mask(x) for x in chroma], roi=small, **RUN)
    with pytest.raises(ValueError) as got:
        run_video_matte(m, frames, key=key, roi=small, **RUN)
    assert str(got.value) == str(want.value) and "does not hold the unknown band" in str(got.value)
    res = run_video_matte(m, _OneShot(frames), key=key, roi=small, **RUN)        # no pre-pass possible: taken as it is
    assert res["roi"] == [small] * T_ and res["roi_size"] == small[2:] and tuple(res["alpha"].shape) == (T_, H_, W_)


def test_key_route_with_roi_auto_reads_a_y4m_file_twice(route, tmp_path):
    from otvm_amd import keys, yuv
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    path = str(tmp_path / "clip.y4m")
    with open(path, "wb") as f:
        f.write(yuv.format_y4m_header(W_, H_, "25:1", C="420mpeg2"))
        for fr in frames:
            f.write(b"FRAME\n" + Y.pack_frame(*Y.rgb_to_yuv420(fr, "601", "limited", rgb=False)))
    key = keys.ChromaKey("green", **KEY_KW)
    src = yuv.Y4MFrames(path, DEV, depth=3)
    assert src.rereadable is True
    host = []
    for t in range(T_):
        d = src[t]
        d._otvm_ready.synchronize()
        host.append(d.cpu().numpy())
    kw = dict(RUN, frames_are_rgb=True, roi="auto", roi_margin=8)
    got = run_video_matte(m, src, key=key, **kw)                                   # the pre-pass, then the loop from frame 0 again
    src.close()
    want = run_video_matte(m, host, key=key, **kw)
    _same(got, want)
    assert (got["roi"], got["roi_size"], got["roi_clipped"]) == (want["roi"], want["roi_size"], want["roi_clipped"])
    assert len(set(got["roi"])) > 1
    with open(path, "rb") as f:
        pipe = yuv.Y4MFrames(_Unseekable(f), DEV, frames=T_)
        assert pipe.rereadable is False
        with pytest.raises(ValueError, match="roi='auto'.*window"):
            run_video_matte(m, pipe, key=key, **kw)
        pipe.close()


class _Unseekable:
    """A file that behaves as a pipe does"""

    def __init__(self, f):
        self.f = f

    def seekable(self):
        return False

    def readline(self, n=-1):
        return self.f.readline(n)

    def readinto(self, b):
        return self.f.readinto(b)


def test_propagating_from_a_keyed_first_frame(route):
    from otvm_amd import keys
    from otvm_amd.masks import Mask
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    f0 = torch.from_numpy(frames[0]).to(DEV)
    keyed = keys.key_mask(f0, keys.ChromaKey("green", **KEY_KW)).cpu()
    assert np.array_equal(keyed.numpy(), chroma[0])
    got = run_video_matte(m, frames, mask=Mask(keyed), **RUN)
    want = run_video_matte(m, frames, mask=Mask(chroma[0]), **RUN)
    for k in ("alpha", "alpha_u8", "trimap"):
        assert torch.equal(got[k], want[k]), k
    assert got["bank_frames"] == want["bank_frames"] and any(got["bank_frames"])       # this one DOES propagate


# ------------------------------------------------------------------------------------------------ command lines
def test_eval_cli_key_writes_what_the_python_call_returns(route, tmp_path):
    from PIL import Image
    from otvm_amd import eval_cli, keys
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    demo = os.path.join(str(tmp_path), "demo")
    os.makedirs(os.path.join(demo, "clip", "frames"))
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames]
    for t in range(T_):
        Image.fromarray(rgb[t]).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
    ppath = os.path.join(str(tmp_path), "plate.png")
    Image.fromarray(np.ascontiguousarray(plate[..., ::-1])).save(ppath)
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "2"]

    def pngs(out):
        d = os.path.join(out, "alpha", "test", "s4_OTVM", "pred", "clip")
        return [np.asarray(Image.open(os.path.join(d, "%04d.png" % t))) for t in range(T_)]
    out, sj = os.path.join(str(tmp_path), "out_key"), os.path.join(str(tmp_path), "key.json")
    res = eval_cli.main(common + ["--out", out, "--key", "green", "--mask-band", "9", "--summary-json", sj])
    assert res["frames"] == T_ and json.load(open(sj))["key"] == "green"
    ref = run_video_matte(m, rgb, key=keys.ChromaKey("green", band=9.0), frames_are_rgb=True, skip=2, max_num=5)
    for t, a in enumerate(pngs(out)):
        assert np.array_equal(a, ref["alpha_u8"][t].numpy()), t
    out = os.path.join(str(tmp_path), "out_plate")
    eval_cli.main(common + ["--out", out, "--plate", ppath, "--plate-thresholds", "10,36", "--plate-radius", "2", "--roi", "auto"])
    ref = run_video_matte(m, frames, key=keys.PlateKey(plate, lo=10, hi=36, radius=2), roi="auto", skip=2, max_num=5)
    for t, a in enumerate(pngs(out)):
        assert np.array_equal(a, ref["alpha_u8"][t].numpy()), t


def test_y4m_cli_key_needs_no_art(route, tmp_path):
    from otvm_amd import keys, yuv
    from otvm_amd.video import run_video_matte
    m, frames, plate, chroma, plated = route
    path, apath = str(tmp_path / "clip.y4m"), str(tmp_path / "alpha.y4m")
    with open(path, "wb") as f:
        f.write(yuv.format_y4m_header(W_, H_, "25:1", C="420mpeg2"))
        for fr in frames:
            f.write(b"FRAME\n" + Y.pack_frame(*Y.rgb_to_yuv420(fr, "601", "limited", rgb=False)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["OTVM_AUTOTUNE"] = "0"                                                        # as the fixture's engine.AUTOTUNE = False
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "otvm_amd.y4m_cli", path, "--key", "green", "--alpha", apath, "--synthetic-weights",
                        "--skip", "2", "--max-num", "3"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["frames"] == T_
    data = open(apath, "rb").read()
    h = yuv.parse_y4m_header(data)
    body, n = data[h.length:], 6 + H_ * W_
    assert (h.W, h.H, h.C) == (W_, H_, "mono") and len(body) == T_ * n
    src = yuv.Y4MFrames(path, DEV)
    ref = run_video_matte(m, src, key=keys.ChromaKey("green"), frames_are_rgb=True, **RUN)
    src.close()
    assert ref["bank_frames"] == [[]] * T_
    for t in range(T_):
        assert body[t * n:t * n + 6] == b"FRAME\n" and body[t * n + 6:(t + 1) * n] == ref["alpha_u8"][t].numpy().tobytes(), t
    assert 0 < float((ref["alpha_u8"] > 0).float().mean()) < 1
