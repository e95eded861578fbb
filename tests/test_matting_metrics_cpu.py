"""Grad and Conn matting metrics, CPU side: the restatement (tests/matting_metrics_ref.py) against the reference's own values
(tests/golden/metrics_grad_conn.npz, tests/golden/make_metric_golden.py) and the library's host-side constants."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import matting_metrics_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_grad_conn.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def _frames(fx):
    return [(str(n), fx["pred_%d" % i], fx["target_%d" % i], fx["mask_%d" % i]) for i, n in enumerate(fx["names"])]


def test_restatement_reproduces_reference_grad_and_conn(fx):
    """Grad within 1e-4 relative (the reference filters in float32), Conn within 1e-5 relative of the reference's float32
    sums; the frames include the equal-size tie in both raster orders, where only the right winner gives the value."""
    for i, (name, p, t, m) in enumerate(_frames(fx)):
        g, c = R.grad(p, t, m), R.conn(p, t, m)
        gr, cr = float(fx["grad"][i]), float(fx["conn"][i])
        assert abs(g - gr) <= 1e-4 * abs(gr) + 1e-6, (name, g, gr)
        assert abs(c - cr) <= 1e-5 * abs(cr) + 1e-6, (name, c, cr)
    blobs = {n: float(fx["conn"][i]) for i, n in enumerate(fx["names"])}
    assert blobs["blobs0"] != blobs["blobs1"]


def test_restatement_levels_match_reference_thresholds(fx):
    assert np.array_equal(R.levels(), fx["levels"]) and np.array_equal(R.levels(), torch.arange(0, 1.1, 0.1).numpy())
    x = np.arange(256)[:, None]
    assert np.array_equal(x >= R.cutoffs()[None, :], fx["passes"])


def test_library_cutoffs_levels_and_taps():
    """The kernel's host-side constants (otvm_matting_grad_conn_params): the cutoffs agree with the reference's float32
    comparison u8 / 255. >= t_i for all 256 values, the levels with torch.arange bit for bit, the filter taps with
    genGaussKernel's factors."""
    import __graft_entry__ as g
    g.build()
    from otvm_amd import lib as L
    lib = L.load()
    cut = (C.c_int * 10)()
    lev = (C.c_float * 11)()
    taps = (C.c_double * 18)()
    L.check(lib.otvm_matting_grad_conn_params(cut, lev, taps), "matting_grad_conn_params")
    steps = torch.arange(0, 1 + 0.1, 0.1)                       # metric.py:215
    assert np.array_equal(np.frombuffer(lev, np.float32), steps.numpy())
    x = torch.arange(256).float() / 255.
    for i in range(1, 11):
        passes = (x >= steps[i]).numpy()
        assert np.array_equal(np.arange(256) >= cut[i - 1], passes), i
    assert list(cut) == list(R.cutoffs())
    gr, dgr = R.grad_taps()
    assert np.allclose(np.frombuffer(taps, np.float64), np.concatenate([gr, dgr]), rtol=1e-14, atol=1e-16)
    hx = np.outer(gr, dgr)                                      # genGaussKernel's hx: unit L2 norm, antisymmetric in j
    assert abs(np.sqrt((hx ** 2).sum()) - 1.0) < 1e-12 and np.allclose(hx, -hx[:, ::-1], atol=0)
    assert L.load().otvm_matting_grad_conn_ws_bytes(1080, 1920) >= 9 * 1080 * 1920
