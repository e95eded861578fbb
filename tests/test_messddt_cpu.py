"""MESSDdt and its Farneback flow, CPU side: the restatement (tests/farneback_ref.py) against the reference's own MESSDdt
(tests/golden/metrics_messddt.npz, tests/golden/make_messddt_golden.py), the pyramid level table, the flow's axis and sign
convention, and the library's host-side constants (otvm_optflow_farneback_params, ABI 21)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import farneback_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_messddt.npz")

# (H, W) -> levels k = L .. 0 as (width, height, GaussianBlur ksize)
LEVEL_TABLE = {
    (1080, 1920): [(60, 34, 79), (120, 68, 39), (240, 135, 19), (480, 270, 9), (960, 540, 3), (1920, 1080, 3)],
    (480, 832): [(104, 60, 19), (208, 120, 9), (416, 240, 3), (832, 480, 3)],
    (2160, 3840): [(120, 68, 79), (240, 135, 39), (480, 270, 19), (960, 540, 9), (1920, 1080, 3), (3840, 2160, 3)],
    (96, 128): [(64, 48, 3), (128, 96, 3)],
    (48, 64): [(64, 48, 3)],
}


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def _clips(fx):
    return [(str(n), fx["pred_%d" % i], fx["target_%d" % i], i) for i, n in enumerate(fx["names"])]


def _lib():
    import __graft_entry__ as g
    g.build()
    from otvm_amd import lib as L
    return L, L.load()


def test_restatement_reproduces_reference_messddt(fx):
    """Per pair: the restatement's MESSDdt (cv2's float32 flow restated, the transposed lookup, exact integer sums) equals
    the reference's float64 values to 1e-12 relative and its float32 values within 2 |ref32 - ref64| + 1e-9; the rounded
    flows equal the fixture's."""
    for name, p, t, ci in _clips(fx):
        flows = [F.farneback(t[i], t[i + 1], np.float32) for i in range(len(t) - 1)]
        for i, f in enumerate(flows):
            assert np.array_equal(F.rint_flow(f), fx["flow_%d" % ci][i].astype(np.int64)), (name, i)
        err, num = F.messddt(p, t, None, flows)
        e64, n64 = fx["err64_%d" % ci], fx["num64_%d" % ci]
        e32, n32 = fx["err32_%d" % ci].astype(np.float64), fx["num32_%d" % ci].astype(np.float64)
        assert len(err) == len(e64) == len(t) - 1
        assert np.all(np.abs(err - e64) <= 1e-12 * np.abs(e64)), (name, err, e64)
        assert np.array_equal(num, n64), (name, num, n64)
        assert np.all(np.abs(err - e32) <= 2 * np.abs(e32 - e64) + 1e-9), (name, err, e32)
        assert np.all(np.abs(num - n32) <= 2 * np.abs(n32 - n64) + 1e-9), (name, num, n32)


def test_fixture_covers_transposition_stillness_and_level_counts(fx):
    """The non-square clip's transposed lookup gives another value than the straight one (so the fixture tells them apart),
    the still clip has zero flow, and the clips span level counts 0 .. 3."""
    names = {n: (p, t, ci) for n, p, t, ci in _clips(fx)}
    p, t, ci = names["nonsq_l0"]
    H, W = t.shape[1:]
    assert H != W
    fl = fx["flow_%d" % ci][0].astype(np.int64)
    r, c = np.mgrid[:H, :W]
    straight = np.clip(r + fl[..., 1], 0, H - 1) * W + np.clip(c + fl[..., 0], 0, W - 1)
    assert not np.array_equal(straight, F.warp_index(fl, H, W))
    m = F.unknown_mask(t)
    e_t = F.messddt_pair(p[0], t[0], m[0], p[1], t[1], m[1], fl)[0]
    i64 = lambda a: np.asarray(a, np.int64)
    e1 = (i64(p[1]).ravel()[straight] - i64(t[1]).ravel()[straight]) ** 2 * m[1].ravel()[straight]
    e_s = int(np.abs((i64(p[0]) - i64(t[0])) ** 2 * m[0] - e1).sum()) / 255.0 ** 2
    assert abs(e_t - float(fx["err64_%d" % ci][0])) <= 1e-12 * e_t and e_s != e_t
    _, t, ci = names["still"]
    assert not np.any(fx["flow_%d" % ci]) and not np.any(F.farneback(t[0], t[1], np.float32))
    counts = sorted(len(F.level_table(*fx["target_%d" % i].shape[1:])) - 1 for i in range(len(fx["names"])))
    assert set(counts) == {0, 1, 2, 3}


def test_restatement_level_table():
    for (H, W), rows in LEVEL_TABLE.items():
        assert [(w, h, ks) for _, w, h, ks, _ in F.level_table(H, W)] == rows, (H, W)
        assert [k for k, *_ in F.level_table(H, W)] == list(range(len(rows) - 1, -1, -1))


def test_library_level_table_and_taps():
    """otvm_optflow_farneback_params: the level table above, the GaussianBlur kernels, the polynomial-expansion taps and the
    flow window taps equal the restatement's float32 constants bit for bit (the inverse moments to 1e-14)."""
    L, lib = _lib()
    assert L.ABI_VERSION == 21 and lib.otvm_abi_version() == 21
    for (H, W), rows in LEVEL_TABLE.items():
        lv = (C.c_int * 24)()
        bt = (C.c_float * (6 * 79))()
        pt = (C.c_float * 24)()
        pi = (C.c_double * 4)()
        wt = (C.c_float * 6)()
        n = lib.otvm_optflow_farneback_params(H, W, lv, bt, pt, pi, wt)
        assert n == len(rows)
        got = np.frombuffer(lv, np.int32)[:4 * n].reshape(n, 4)
        assert [tuple(r[1:]) for r in got.tolist()] == rows and got[:, 0].tolist() == list(range(n - 1, -1, -1))
        taps = np.frombuffer(bt, np.float32).reshape(6, 79)
        for i, (k, w, h, ks, sigma) in enumerate(F.level_table(H, W)):
            want = F.gaussian_kernel(ks, sigma if k > 0 else 0.0, np.float32)
            assert np.array_equal(taps[i, :ks], want) and not taps[i, ks:].any(), (H, W, k)
        g, xg, xxg, ig = F.poly_taps(np.float32)
        p = np.frombuffer(pt, np.float32).reshape(3, 8)
        assert np.array_equal(p[0], g[7:]) and np.array_equal(p[1], xg[7:]) and np.array_equal(p[2], xxg[7:])
        assert np.allclose(np.frombuffer(pi, np.float64), ig, rtol=1e-14, atol=0)
        assert np.array_equal(np.frombuffer(wt, np.float32), F.window_taps(np.float32))
    assert lib.otvm_optflow_farneback_params(0, 5, None, None, None, None, None) == -1
    assert lib.otvm_optflow_farneback_ws_bytes(1080, 1920) >= 4 * 20 * 1080 * 1920


def test_library_exports_messddt_symbols():
    L, lib = _lib()
    for s in ("otvm_optflow_farneback", "otvm_optflow_farneback_ws_bytes", "otvm_optflow_farneback_params", "otvm_matting_messddt"):
        assert hasattr(lib, s), s


def test_poly_inverse_closed_form():
    """The closed-form entries of the inverse moment matrix equal a general inverse."""
    _, _, _, ig = F.poly_taps(np.float64)
    n = F.POLY_N
    xs = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-xs ** 2 / (2 * F.POLY_SIGMA ** 2))
    g /= g.sum()
    G = np.zeros((6, 6))
    gg = np.outer(g, g)
    X, Y = np.meshgrid(xs, xs)
    G[0, 0] = gg.sum()
    G[1, 1] = G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = (gg * X * X).sum()
    G[3, 3] = G[4, 4] = (gg * X ** 4).sum()
    G[3, 4] = G[4, 3] = G[5, 5] = (gg * X * X * Y * Y).sum()
    iG = np.linalg.inv(G)
    assert np.allclose(ig, (iG[1, 1], iG[0, 3], iG[3, 3], iG[5, 5]), rtol=1e-9)


def test_flow_axis_and_sign():
    """A smooth textured image moved by (dx, dy) = (3, -2): the restatement's median flow over the interior is within 0.1 px
    of (3, -2), channel 0 = dx (horizontal), channel 1 = dy -- the convention the reference's transposed lookup rests on."""
    from scipy import ndimage
    rng = np.random.default_rng(0)
    H, W, pad = 256, 320, 20
    base = ndimage.gaussian_filter(rng.standard_normal((H + 2 * pad, W + 2 * pad)), 4.0)
    base = (base - base.min()) / (base.max() - base.min()) * 255
    a = base[pad:pad + H, pad:pad + W]
    b = base[pad + 2:pad + 2 + H, pad - 3:pad - 3 + W]          # next(y, x) = prev(y + 2, x - 3): content moves by (+3, -2)
    f = F.farneback(np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8), np.float32)
    inner = f[40:-40, 40:-40]
    med = (float(np.median(inner[..., 0])), float(np.median(inner[..., 1])))
    print("median flow", med)
    assert abs(med[0] - 3) <= 0.1 and abs(med[1] + 2) <= 0.1
