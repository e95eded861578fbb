"""CPU: the masks of keyed footage -- the restatement of both kernels (tests/key_ref.py) against the float64 definition, the
properties of the two keys, and the argument rules of keys.py, run_video_matte(key=...), eval_cli and y4m_cli that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import key_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEN, BLUE, TEAL = (0, 255, 0), (0, 0, 255), (20, 170, 150)


def _pixels():
    """All of a 64^3 RGB lattice (both ends of the range included) plus random pixels"""
    v = np.round(np.linspace(0, 255, 64)).astype(np.int64)
    lat = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    rnd = np.random.default_rng(7).integers(0, 256, (200000, 3))
    return np.concatenate([lat, rnd])


# ------------------------------------------------------------------------------------------------ restatement vs definition
def test_chroma_stage_is_within_one_code_value_of_the_definition():
    """DERIVED, not measured: a 20-bit coefficient is off by at most 2^-21, three of them at 8-bit operands by less than
    3 x 255 x 2^-21 < 0.001 code values, so the integer sum and the exact one round to different integers only when the exact
    value lies within 0.001 of a tie -- and then by exactly one."""
    px = _pixels()
    R, G, B = px[:, 0], px[:, 1], px[:, 2]
    cb, cr = K.chroma_int(R, G, B)
    db, dr = K.chroma_def(R, G, B)
    eb, er = K.chroma_exact(R, G, B)
    for got, want, exact in ((cb, db, eb), (cr, dr, er)):
        diff = np.abs(got - want)
        assert diff.max() <= 1
        frac = np.abs((exact + 0.5) - np.round(exact + 0.5))          # distance of the exact value from a rounding tie
        exact_clamped = (exact <= -0.5) | (exact >= 255.5)
        assert (frac[(diff == 1) & ~exact_clamped] < 0.001).all()
    # grey has no chroma, exactly, and the primaries sit where the standard puts them
    g = np.arange(256)
    assert all((c == 0).all() for c in K.chroma_int(g, g, g))
    assert K.key_chroma(GREEN) == (-84, -107) and K.key_chroma(BLUE) == (127, -21) and K.key_chroma((255, 0, 0)) == (-43, 127)


@pytest.mark.parametrize("colour", [GREEN, BLUE, TEAL])
@pytest.mark.parametrize("lo,hi", [(8, 24), (0, 1), (-3, 40), (10, 10.01)])
def test_after_the_chroma_stage_the_restatement_is_exact(colour, lo, hi):
    kb, kr = K.key_chroma(colour)
    qlo, qhi = K.thresholds(kb, kr, lo, hi)
    assert qlo < qhi
    px = _pixels()[::37]
    cb, cr = K.chroma_int(px[:, 0], px[:, 1], px[:, 2])
    got = K.ramp_down(K.cone(cb, cr, kb, kr), qlo, qhi)
    assert np.array_equal(got, K.mask_from_cone_def(cb, cr, kb, kr, qlo, qhi))
    assert np.array_equal(got, K.mask_from_chroma(px[None], kb, kr, qlo, qhi, rgb=True)[0])
    assert np.array_equal(got, K.mask_from_chroma(px[None, :, ::-1], kb, kr, qlo, qhi, rgb=False)[0])


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_plate_restatement_equals_brute_force(radius):
    g = np.random.default_rng(11 + radius)
    for (H, W), (lo, hi) in (((1, 1), (0, 255)), ((1, 9), (12, 40)), ((9, 1), (12, 13)), ((7, 10), (0, 1)), ((12, 11), (30, 200))):
        plate = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        near = np.clip(plate.astype(int) + g.integers(-45, 46, plate.shape), 0, 255).astype(np.uint8)   # spans both thresholds
        for frame in (near, g.integers(0, 256, (H, W, 3), dtype=np.uint8)):
            assert np.array_equal(K.mask_from_plate(frame, plate, radius, lo, hi), K.mask_from_plate_def(frame, plate, radius, lo, hi))


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("colour", [GREEN, BLUE, TEAL])
def test_pure_key_pixels_are_screen_at_any_brightness_that_clears_hi(colour):
    kb, kr = K.key_chroma(colour)
    lo, hi = 8, 24
    qlo, qhi = K.thresholds(kb, kr, lo, hi)
    scales = np.arange(1, 256) / 255.0
    px = np.floor(np.asarray(colour)[None] * scales[:, None] + 0.5).astype(np.int64)
    q = K.cone(*K.chroma_int(px[:, 0], px[:, 1], px[:, 2]), kb, kr)
    clears = q >= qhi                                             # which brightnesses are saturated enough: computed, not assumed
    assert clears.sum() > 150 and clears[-1]
    m = K.ramp_down(q, qlo, qhi)
    assert (m[clears] == 0).all()
    # brightness alone never makes a subject of the screen: along the ray q grows with the scale, up to the rounding of Cb, Cr
    # (one code value each: |dq| <= 2 (|kb| + |kr|))
    assert (np.diff(q) >= -2 * (abs(kb) + abs(kr))).all()


@pytest.mark.parametrize("colour", [GREEN, BLUE, TEAL])
def test_every_grey_is_subject_and_the_mask_is_monotone_in_q(colour):
    kb, kr = K.key_chroma(colour)
    qlo, qhi = K.thresholds(kb, kr, 8, 24)
    g = np.arange(256, dtype=np.uint8)
    grey = np.stack([g, g, g], -1)[None]
    assert (K.mask_from_chroma(grey, kb, kr, qlo, qhi) == 255).all()
    q = np.arange(qlo - 50, qhi + 50)
    m = K.ramp_down(q, qlo, qhi).astype(int)
    assert (np.diff(m) <= 0).all() and m[0] == 255 and m[-1] == 0
    assert m[q == qlo][0] == 255 and m[q == qhi][0] == 0 and m[q == qlo + 1][0] == 255 - 255 // (qhi - qlo)
    d = np.arange(256)
    u = K.ramp_up(d, 12, 40).astype(int)
    assert (np.diff(u) >= 0).all() and u[12] == 0 and u[40] == 255 and u[13] == 255 // 28


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_a_frame_that_is_its_plate_is_all_plate(radius):
    f = np.random.default_rng(3).integers(0, 256, (13, 17, 3), dtype=np.uint8)
    assert (K.mask_from_plate(f, f, radius, 0, 1) == 0).all()
    # and the neighbourhood absorbs a one-pixel shift when radius >= 1
    shifted = np.roll(f, 1, axis=1)
    m = K.mask_from_plate(shifted, f, radius, 0, 1)
    assert (m[:, 1:] == 0).all() if radius >= 1 else (m == 255).any()


# ------------------------------------------------------------------------------------------------ keys.py
def test_key_objects_hold_the_restatements_integers():
    from otvm_amd import keys
    for colour, name in ((GREEN, "green"), (BLUE, "blue"), (TEAL, TEAL)):
        k = keys.ChromaKey(name, lo=6.5, hi=30)
        assert (k.kb, k.kr) == K.key_chroma(colour) == keys.chroma_of(colour)
        assert (k.qlo, k.qhi) == K.thresholds(k.kb, k.kr, 6.5, 30)
        assert (k.band, k.mask_lo, k.mask_hi) == (None, 127, 128)
    px = np.random.default_rng(5).integers(0, 256, (500, 3))
    assert all(keys.chroma_of(p) == tuple(int(v[0]) for v in K.chroma_int(p[0:1], p[1:2], p[2:3])) for p in px)
    p = keys.PlateKey(np.zeros((4, 6, 3), np.uint8), lo=3, hi=9, radius=2, band=5, mask_lo=10, mask_hi=200)
    assert (p.lo, p.hi, p.radius, p.shape, p.band, p.mask_lo, p.mask_hi) == (3, 9, 2, (4, 6), 5, 10, 200)
    assert keys.PlateKey(torch.zeros((4, 6, 3), dtype=torch.uint8)).shape == (4, 6)
    assert "PLACEHOLDER" in keys.ChromaKey.__doc__ and "PLACEHOLDER" in keys.PlateKey.__doc__ and "PLACEHOLDER" in keys.__doc__


def test_key_objects_refuse_bad_arguments():
    from otvm_amd import keys
    for colour in ((128, 128, 128), (0, 0, 0), (200, 190, 195), "red", (1, 2), (0, 256, 0), (0.5, 3, 4)):
        with pytest.raises(ValueError, match="colour"):
            keys.ChromaKey(colour)
    for lo, hi in ((24, 8), (8, 8), (8, None), (True, 9), (10, 10.0001), (0, 1000)):
        with pytest.raises(ValueError, match="thresholds"):
            keys.ChromaKey("green", lo=lo, hi=hi)
    plate = np.zeros((4, 6, 3), np.uint8)
    for lo, hi in ((40, 12), (12, 12), (-1, 5), (5, 256), (1.5, 7)):
        with pytest.raises(ValueError, match="thresholds"):
            keys.PlateKey(plate, lo=lo, hi=hi)
    for r in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="radius"):
            keys.PlateKey(plate, radius=r)
    for bad in (np.zeros((4, 6), np.uint8), np.zeros((4, 6, 3), np.float32), np.zeros((4, 6, 4), np.uint8), [[1, 2, 3]]):
        with pytest.raises(ValueError, match="plate"):
            keys.PlateKey(bad)
    with pytest.raises(ValueError, match="band"):
        keys.ChromaKey("green", band=300)
    with pytest.raises(ValueError, match="thresholds"):
        keys.ChromaKey("green", mask_lo=128, mask_hi=128)
    with pytest.raises(ValueError, match="GPU"):
        keys.key_mask(torch.zeros((4, 6, 3), dtype=torch.uint8), keys.ChromaKey("green"))
    with pytest.raises(ValueError, match="ChromaKey"):
        keys.key_mask(torch.zeros((4, 6, 3), dtype=torch.uint8), "green")


# ------------------------------------------------------------------------------------------------ run_video_matte(key=...)
class _NoDevice(torch.nn.Module):
    """Stands where the model does: the argument rules are checked before any device work."""
    DILATION_KERNEL = 12

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


class _OneShot:
    """A source that is read once, in order (a pipe)"""

    def __init__(self, frames):
        self.it, self.n, self.i = iter(frames), len(frames), 0

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        assert i == self.i, "read in order, once"
        self.i += 1
        return next(self.it)


def test_run_video_matte_refuses_before_anything_is_uploaded():
    from otvm_amd import keys
    from otvm_amd.subjects import run_video_matte_subjects
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    model = _NoDevice()
    H, W, T = 6, 8, 3
    frames = [np.zeros((H, W, 3), np.uint8)] * T
    m, tri = np.zeros((H, W), np.uint8), np.zeros((3, H, W), np.float32)
    key = keys.ChromaKey("green")
    for kw, word in ((dict(trimap=tri), "`trimap`"), (dict(mask=m), "`mask`"), (dict(masks=[m] * T), "`masks`"),
                     (dict(keyframes={0: tri}), "`keyframes`"), (dict(alphas=[m] * T), "`alphas`"),
                     (dict(backgrounds=frames), "`backgrounds`"), (dict(roi="track"), "roi='track'"),
                     (dict(roi=("track", 4, 4)), "roi='track'")):
        with pytest.raises(ValueError, match="`key`") as e:
            run_video_matte(model, frames, key=key, **kw)
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError, match="`key`.*ChromaKey"):
        run_video_matte(model, frames, key="green")
    with pytest.raises(ValueError, match="`key`.*float frames"):
        run_video_matte(model, [np.zeros((H, W, 3), np.float32)] * T, key=key)
    with pytest.raises(ValueError, match="plate of `key` is 6x9.*6x8"):
        run_video_matte(model, frames, key=keys.PlateKey(np.zeros((H, W + 1, 3), np.uint8)))
    src = _OneShot(frames)
    with pytest.raises(ValueError, match="`key`.*roi='auto'.*window"):
        run_video_matte(model, src, key=key, roi="auto")
    assert src.i == 0                                                 # refused before a frame was asked for
    model.DILATION_KERNEL = None
    with pytest.raises(ValueError, match="band"):
        run_video_matte(model, frames, key=key)
    with pytest.raises(ValueError, match="run_video_matte_batch: key"):
        run_video_matte_batch(model, [frames], trimaps=[tri], key=key)
    with pytest.raises(ValueError, match="run_video_matte_subjects: key"):
        run_video_matte_subjects(model, frames, [tri], key=key)


def test_y4m_source_says_whether_it_can_be_read_twice():
    from otvm_amd import yuv
    assert isinstance(yuv.Y4MFrames.rereadable, property)


# ------------------------------------------------------------------------------------------------ command lines
def test_cli_parsing(tmp_path):
    import argparse
    from PIL import Image
    from otvm_amd import eval_cli, keys

    def parse(argv):
        ap = argparse.ArgumentParser()
        eval_cli.add_key_arguments(ap)
        return eval_cli.parse_key_options(ap.parse_args(argv))
    assert parse([]) is None
    k = parse(["--key", "green"])(None, 127, 128, 4, 6, True)
    assert isinstance(k, keys.ChromaKey) and k.colour == GREEN and (k.lo, k.hi, k.band) == (8, 24, None)
    k = parse(["--key", "20,170,150", "--key-thresholds", "5,31.5"])((4, 9), 25, 230, 4, 6, False)
    assert k.colour == TEAL and (k.lo, k.hi, k.band, k.mask_lo, k.mask_hi) == (5.0, 31.5, (4, 9), 25, 230)
    plate = np.random.default_rng(2).integers(0, 256, (4, 6, 3), dtype=np.uint8)
    path = str(tmp_path / "plate.png")
    Image.fromarray(plate).save(path)
    make = parse(["--plate", path, "--plate-thresholds", "3,9", "--plate-radius", "2"])
    k = make(None, 127, 128, 4, 6, True)
    assert isinstance(k, keys.PlateKey) and (k.lo, k.hi, k.radius) == (3, 9, 2) and np.array_equal(k.plate, plate)
    assert np.array_equal(make(None, 127, 128, 4, 6, False).plate, plate[..., ::-1])          # B, G, R frames: a B, G, R plate
    with pytest.raises(SystemExit, match="is 6x4, the frames are 6x5"):
        make(None, 127, 128, 5, 6, True)
    for argv, word in ((["--key", "green", "--plate", path], "exclude"), (["--key-thresholds", "1,2"], "belongs"),
                       (["--plate-radius", "1"], "belong"), (["--key", "red"], "--key is"), (["--key", "1,2"], "--key is"),
                       (["--key", "0,300,0"], "--key is"), (["--key", "128,128,128"], "grey"),
                       (["--key", "green", "--key-thresholds", "9,3"], "thresholds"), (["--key", "green", "--key-thresholds", "9"], "LO,HI"),
                       (["--plate", path, "--plate-thresholds", "40,12"], "--plate-thresholds"),
                       (["--plate", path, "--plate-radius", "4"], "--plate-radius"),
                       (["--plate", str(tmp_path / "none.png")], "not an existing image")):
        with pytest.raises(SystemExit) as e:
            parse(argv)
        assert word in str(e.value), (argv, str(e.value))


def test_command_lines_refuse_keys_outside_their_route(tmp_path):
    from otvm_amd import eval_cli, y4m_cli
    data = str(tmp_path)
    for argv, word in ((["--key", "green"], "--demo"), (["--demo", "--key", "green", "--masks", "frame"], "--masks"),
                       (["--demo", "--key", "green", "--keyframes"], "--keyframes"), (["--demo", "--key", "green", "--subjects"], "--subjects"),
                       (["--demo", "--key", "green", "--batch", "2"], "--batch"), (["--demo", "--key", "green", "--roi", "track"], "--roi track"),
                       (["--demo", "--key", "green", "--plate", "p.png"], "exclude"), (["--demo", "--plate", "p.png"], "existing image")):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(["--data", data, "--synthetic-weights"] + argv)
        assert word in str(e.value), (argv, str(e.value))
    base = ["in.y4m", "--alpha", "a.y4m", "--synthetic-weights"]
    for argv, word in (([], "exactly one"), (["--key", "green", "--trimap", "t.png"], "exactly one"),
                       (["--key", "green", "--mask", "m.png"], "exactly one"), (["--key", "green", "--roi", "auto"], "window"),
                       (["--key", "green", "--roi", "track"], "window"), (["--trimap", "t.png", "--roi", "0,0,32,32"], "track"),
                       (["--key", "128,128,128"], "grey"), (["--trimap", "t.png", "--mask-band", "4"], "--mask-band")):
        with pytest.raises(SystemExit) as e:
            y4m_cli.main(base + argv)
        assert word in str(e.value), (argv, str(e.value))


def test_binding_declares_the_key_entry_points():
    import __graft_entry__ as g
    from otvm_amd import lib as L
    h = ctypes.CDLL(g.build())
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    for sym, struct, cls in (("otvm_mask_from_chroma", "otvm_mask_from_chroma_params", L.MaskFromChromaParams),
                             ("otvm_mask_from_plate", "otvm_mask_from_plate_params", L.MaskFromPlateParams)):
        assert sym in L.EXPORTED and getattr(h, sym) is not None
        body = header[header.index("typedef struct %s {" % struct):header.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split("{", 1)[1].split(";"):
            decl = decl.strip()
            if decl:
                names += [n.strip().lstrip("*").strip() for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert names == [f[0] for f in cls._fields_], (names, cls._fields_)
    # refusals need no device: nothing is launched for them
    h.otvm_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_uint8 * 64)()
    ok = dict(frame=ctypes.addressof(buf), mask=ctypes.addressof(buf), H=2, W=2, u8_rgb=1, kb=-84, kr=-107, qlo=100, qhi=300)
    for change in (dict(kb=3, kr=-15), dict(qlo=300, qhi=300), dict(qlo=400), dict(H=0), dict(W=16384), dict(frame=None), dict(mask=None),
                   dict(kb=200), dict(qhi=1 << 21)):
        p = L.MaskFromChromaParams(**{**ok, **change})
        assert h.otvm_mask_from_chroma(ctypes.byref(p), None) != 0, change
        assert h.otvm_last_error().decode().startswith("otvm_mask_from_chroma"), change
    ok = dict(frame=ctypes.addressof(buf), plate=ctypes.addressof(buf), mask=ctypes.addressof(buf), H=2, W=2, radius=1, lo=12, hi=40)
    for change in (dict(radius=-1), dict(radius=4), dict(lo=40, hi=12), dict(lo=12, hi=12), dict(lo=-1), dict(hi=256), dict(H=16384),
                   dict(W=0), dict(plate=None), dict(frame=None), dict(mask=None)):
        p = L.MaskFromPlateParams(**{**ok, **change})
        assert h.otvm_mask_from_plate(ctypes.byref(p), None) != 0, change
        assert h.otvm_last_error().decode().startswith("otvm_mask_from_plate"), change
    assert h.otvm_mask_from_chroma(None, None) != 0 and h.otvm_mask_from_plate(None, None) != 0
