"""Foreground outputs, host side (no GPU): the library's new symbols and struct layout, the numpy restatement of the output
kernel on hand-worked values, and the drivers' new arguments."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import fgr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_fgr_symbols_and_keeps_abi_21(tmp_path):
    from otvm_amd.csrc.build import build
    from otvm_amd import lib as L
    build()
    h = L.load()
    for sym in ("otvm_conv2d_head_fgr", "otvm_fba_head_fgr", "otvm_fgr_outputs"):
        assert sym in L.EXPORTED and getattr(h, sym) is not None
    assert h.otvm_abi_version() == 21 and L.ABI_VERSION == 21
    src = '#include <stdio.h>\n#include "otvm_hip.h"\nint main(){printf("%zu %zu\\n", sizeof(otvm_fgr_params), sizeof(otvm_head_params));return 0;}\n'
    exe = os.path.join(str(tmp_path), "fgr_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    a, b = (int(v) for v in subprocess.check_output([exe]).split())
    assert ctypes.sizeof(L.FgrParams) == a
    assert ctypes.sizeof(L.HeadParams) == b              # untouched by this feature


def test_fgr_ref_hand_worked_bytes():
    f32 = np.float32
    below = lambda k: np.nextafter(f32(k) / f32(255), f32(0))       # just below k/255: truncates to k - 1
    # quantisation: truncation, exact k/255 (k/255 * 255 rounds back to k for every byte value), the top of the range
    assert fgr_ref.quant_u8(f32(0)) == 0 and fgr_ref.quant_u8(f32(1)) == 255
    assert fgr_ref.quant_u8(below(128)) == 127 and fgr_ref.quant_u8(below(1)) == 0 and fgr_ref.quant_u8(below(255)) == 254
    assert fgr_ref.quant_u8(f32(254.999) / f32(255)) == 254
    assert fgr_ref.quant_u8(f32(1) / f32(255)) == 1
    assert list(fgr_ref.quant_u8(np.array([np.nan, np.inf, -np.inf], f32))) == [0, 0, 0]
    # alpha in {0, 1, 1/255, 254.999/255} x F in {0, 1, just below 128/255} x bg in {0, 255}: one pixel per combination
    al = np.array([0, 1, f32(1) / f32(255), f32(254.999) / f32(255)], f32)
    Fv = np.array([0, 1, below(128)], f32)
    A, Fg, Bg = np.meshgrid(al, Fv, np.array([0, 255], np.uint8), indexing="ij")
    shape = A.shape[:2]
    for ib, bgv in enumerate((0, 255)):
        a2, f2 = A[..., ib].astype(f32), Fg[..., ib].astype(f32)
        F3 = np.stack([f2, f2, f2])
        fgr, rgba, comp = fgr_ref.fgr_outputs(a2, F3, bg=(bgv, bgv, bgv), u8_rgb=True)
        assert fgr.dtype == np.float32 and np.array_equal(fgr, F3)
        assert np.array_equal(rgba[..., 3], np.array([[0] * 3, [255] * 3, [1] * 3, [254] * 3], np.uint8))
        assert np.array_equal(rgba[..., 0], np.tile(np.array([0, 255, 127], np.uint8), (4, 1)))
        # alpha = 0 -> the background byte; alpha = 1 -> trunc(F * 255)
        assert np.array_equal(comp[0, :, 0], np.full(3, bgv, np.uint8))
        assert np.array_equal(comp[1, :, 0], np.array([0, 255, 127], np.uint8))
        # alpha = 1/255, by hand in float32.  a = fl(1/255) = 8421505 * 2^-31 (a little ABOVE 1/255).
        #   bg 255: bgf = fl(255 * a) = fl(1 + 5.9e-8) = 1 (half an ulp above 1 is 5.96e-8);
        #           1 - a = (2^31 - 8421505) * 2^-31, rounded to 24 bits = 16711423 * 2^-24 = 254/255 + 2.3e-10;
        #     F = 0: c = 1 - a; c * 255 = 254 + 6e-8 -> fl = 254 (ulp there 1.5e-5) -> byte 254
        #     F = 1: c = fl(a + (1 - a)) = fl(1 + 2^-31) = 1 -> byte 255
        #     F just below 128/255: c = fl(0.00196847 + 0.99607843) = 0.99804691; * 255 = 254.502 -> byte 254
        #   bg 0: c = F * a.  F = 0 -> 0; F = 1 -> fl(255 * a) = 1 (as above) -> byte 1; F below 128/255 -> 0.502 -> byte 0
        want = {0: [0, 1, 0], 255: [254, 255, 254]}[bgv]
        assert list(comp[2, :, 0]) == want, list(comp[2, :, 0])
        # alpha = fl(254.999/255) = 0.99999605, 1 - a = 3.95e-6.
        #   bg 0: trunc(F * a * 255): F = 0 -> 0; F = 1 -> 254.999 -> 254; F below 128/255 -> 127.9995 -> 127
        #   bg 255 (bgf = 1): F = 0 -> 3.95e-6 * 255 = 0.001 -> 0; F = 1 -> a + (1 - a) = 1 exactly -> 255;
        #           F below 128/255 -> (0.5019588 + 0.00000395) * 255 = 128.0005 -> 128
        assert list(comp[3, :, 0]) == {0: [0, 254, 127], 255: [0, 255, 128]}[bgv], list(comp[3, :, 0])
        # never above 255 (the clamp): F = 1, alpha close to 1, white background
        assert comp.max() <= 255
    # the clamp itself: a composite above 1 (F = 1, bg = 255 with float rounding cannot exceed; use out-of-range F) stays 255
    _, rgba, comp = fgr_ref.fgr_outputs(np.full((1, 1), 0.5, f32), np.full((3, 1, 1), 3.0, f32), bg=(255, 255, 255))
    assert rgba[0, 0, 0] == 255 and comp[0, 0, 0] == 255
    # channel order: B, G, R by default, R, G, B with u8_rgb; the background follows the output's order
    F3 = np.stack([np.full(shape, v, f32) for v in (0.25, 0.5, 0.75)])
    _, bgr, cb = fgr_ref.fgr_outputs(np.ones(shape, f32), F3, bg=(10, 20, 30))
    _, rgb, _ = fgr_ref.fgr_outputs(np.ones(shape, f32), F3, u8_rgb=True)
    assert list(rgb[0, 0]) == [63, 127, 191, 255] and list(bgr[0, 0]) == [191, 127, 63, 255] and list(cb[0, 0]) == [191, 127, 63]
    _, _, c0 = fgr_ref.fgr_outputs(np.zeros(shape, f32), F3, bg=(10, 20, 30))
    assert list(c0[0, 0]) == [10, 20, 30]
    # non-finite operands give byte 0, only where they enter
    F3n = F3.copy(); F3n[0, 0, 0] = np.nan
    an = np.ones(shape, f32); an[1, 1] = np.inf
    _, rgba, comp = fgr_ref.fgr_outputs(an, F3n, bg=(10, 20, 30), u8_rgb=True)
    assert list(rgba[0, 0]) == [0, 127, 191, 255] and list(comp[0, 0]) == [0, 127, 191]
    assert rgba[1, 1, 3] == 0 and list(comp[1, 1]) == [0, 0, 0] and list(rgba[1, 1, :3]) == [63, 127, 191]


def test_drivers_accept_the_foreground_arguments(monkeypatch):
    from otvm_amd import eval_cli, io_pipeline, video
    from otvm_amd.alpha_model import EvalModel
    for fn in (video.run_video_matte, video.run_video_matte_batch):
        sig = inspect.signature(fn)
        assert sig.parameters["foreground"].default is False and sig.parameters["new_background"].default is None
    assert "bgr" in inspect.signature(io_pipeline.AlphaWriter.put).parameters
    assert hasattr(EvalModel, "set_background")
    assert eval_cli.parse_composite(None) == (None, None)
    assert eval_cli.parse_composite("0,255,0") == ((0, 255, 0), None)
    with pytest.raises(SystemExit):
        eval_cli.parse_composite("0,256,0")
    with pytest.raises(SystemExit):
        eval_cli.parse_composite("/nonexistent/background.png")
    # argparse level: the options exist (parsing stops at the missing --data)
    seen = {}

    class Stop(Exception):
        pass
    import argparse
    orig = argparse.ArgumentParser.parse_args

    def spy(self, argv=None):
        ns = orig(self, argv)
        seen.update(vars(ns))
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(Stop):
        eval_cli.main(["--demo", "--data", "x", "--fgr", "--composite", "0,255,0"])
    assert seen["fgr"] is True and seen["composite"] == "0,255,0"
