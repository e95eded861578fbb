"""Grad and Conn matting metrics on the device (otvm_matting_grad_conn, csrc/metrics_grad_conn.hip) against the reference's
values (tests/golden/metrics_grad_conn.npz) and the CPU restatement (tests/matting_metrics_ref.py): the Conn level map
exactly, at tile-straddling sizes up to 3840x2160; and the layers above it (ClipMetrics, run_sharded, eval_cli)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import matting_metrics_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_grad_conn.npz")


def _lib():
    from otvm_amd import lib as L
    return L, L.load()


def device_grad_conn(p, t, m=None):
    """(grad, conn, level_map) of one frame through the C ABI."""
    L, lib = _lib()
    H, W = p.shape
    dp = torch.from_numpy(np.ascontiguousarray(p)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(t)).cuda()
    dm = None if m is None else torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).cuda()
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    lev = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    ws = torch.empty(lib.otvm_matting_grad_conn_ws_bytes(H, W), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.otvm_matting_grad_conn(dp.data_ptr(), dt.data_ptr(), 0 if dm is None else dm.data_ptr(), H, W, acc.data_ptr(),
                                       lev.data_ptr(), ws.data_ptr(), st), "matting_grad_conn")
    torch.cuda.synchronize()
    a = acc.cpu().tolist()
    return a[0], a[1], lev.cpu().numpy()


def _check_against_restatement(p, t, m, what):
    g, c, lev = device_grad_conn(p, t, m)
    ref_lev = R.conn_level_map(p, t)
    assert np.array_equal(lev, ref_lev), "%s: level map differs at %d pixels" % (what, int((lev != ref_lev).sum()))
    c_ref = float((R.conn_terms(p, t, ref_lev).astype(np.float64) * (1 if m is None else (m != 0))).sum())
    assert abs(c - c_ref) <= 1e-12 * abs(c_ref), (what, c, c_ref)
    g_ref = R.grad(p, t, m)
    assert abs(g - g_ref) <= 1e-6 * abs(g_ref) + 1e-12, (what, g, g_ref)
    return g, c


def test_kernel_reproduces_reference_fixture():
    fx = np.load(GOLDEN)
    worst_g = worst_c = 0.0
    for i, name in enumerate(fx["names"]):
        p, t, m = fx["pred_%d" % i], fx["target_%d" % i], fx["mask_%d" % i]
        g, c = _check_against_restatement(p, t, m, str(name))
        gr, cr = float(fx["grad"][i]), float(fx["conn"][i])
        assert abs(g - gr) <= 1e-4 * abs(gr) + 1e-6, (str(name), g, gr)
        assert abs(c - cr) <= 1e-5 * abs(cr) + 1e-6, (str(name), c, cr)
        worst_g = max(worst_g, abs(g - gr) / max(abs(gr), 1e-30))
        worst_c = max(worst_c, abs(c - cr) / max(abs(cr), 1e-30))
    print("fixture margins: Grad rel %.3e, Conn rel %.3e" % (worst_g, worst_c))


def _field(rng, H, W, sigma):
    """A smooth random alpha pair (components of every size that cross tile edges) with noisy pixels."""
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma, mode="wrap")
    f = (f - f.min()) / max(1e-12, f.max() - f.min())
    t = np.clip(np.rint(f * 290 - 20), 0, 255).astype(np.uint8)
    p = np.clip(t.astype(np.int32) + rng.integers(-40, 41, (H, W)), 0, 255).astype(np.uint8)
    return p, t


@pytest.mark.parametrize("H,W,sigma", [(37, 53, 3.0), (1, 4097, 20.0), (4097, 1, 20.0), (33, 65, 1.0), (96, 160, 0.0),
                                       (200, 300, 6.0)])
def test_level_map_at_tile_straddling_sizes(H, W, sigma):
    rng = np.random.Generator(np.random.PCG64(H * 7919 + W))
    if sigma > 0:
        p, t = _field(rng, H, W, sigma)
    else:                                               # white noise: many small components and ties
        p, t = rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)
    m = (rng.uniform(size=(H, W)) < 0.8).astype(np.uint8)
    _check_against_restatement(p, t, m, "%dx%d" % (H, W))
    _check_against_restatement(p, t, None, "%dx%d unmasked" % (H, W))


@pytest.mark.parametrize("H,W", [(1080, 1920), (2160, 3840)])
def test_level_map_full_size(H, W):
    rng = np.random.Generator(np.random.PCG64(H + W))
    p, t = _field(rng, H, W, 24.0)
    _check_against_restatement(p, t, ((t > 0) & (t < 255)).astype(np.uint8), "%dx%d" % (H, W))


def test_clip_metrics_image_metrics():
    """ClipMetrics(image_metrics=True): per-frame Grad / Conn equal the direct kernel calls, SSDA follows metric.py:244-250,
    and the SAD / MSE / dtSSD keys are those of image_metrics=False."""
    from otvm_amd.video import ClipMetrics
    rng = np.random.Generator(np.random.PCG64(5))
    H, W, T = 70, 90, 4
    frames = [_field(rng, H, W, 5.0) for _ in range(T)]
    plain, full = ClipMetrics("cuda"), ClipMetrics("cuda", capacity=2, image_metrics=True)   # (also grows the buffers)
    for p, t in frames:
        dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
        plain.add(dp, dt, "unknown")
        full.add(dp, dt, "unknown")
    a, b = plain.result(), full.result()
    for k, v in a.items():
        assert b[k] == v, k
    assert set(b) - set(a) == {"grad_per_frame", "conn_per_frame", "grad_sum", "conn_sum", "ssda_per_frame", "ssda_num_per_frame"}
    for i, (p, t) in enumerate(frames):
        m = ((t > 0) & (t < 255)).astype(np.uint8)
        g, c, _ = device_grad_conn(p, t, m)
        assert b["grad_per_frame"][i] == g and b["conn_per_frame"][i] == c, i
        e = ((p.astype(np.float64) - t) / 255.0) ** 2 * m
        assert abs(b["ssda_per_frame"][i] - np.sqrt(e.sum())) <= 1e-12 * np.sqrt(e.sum())
        assert b["ssda_num_per_frame"][i] == m.sum() + 1.0
    assert b["grad_sum"] == pytest.approx(sum(b["grad_per_frame"]), rel=1e-15)
    assert b["conn_sum"] == sum(b["conn_per_frame"])


def test_eval_cli_all_metrics(tmp_path, monkeypatch):
    """eval_cli --all-metrics over a small VideoMatting108 tree reports grad_mean / conn_mean = the per-frame means of the
    per-clip sums; without the flag the summary has today's keys; --batch 2 reports the same means."""
    from otvm_amd import engine, eval_cli
    from tests.test_gpu_multirank import _v108_tree
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    root = os.path.join(str(tmp_path), "data")
    os.makedirs(root)
    _v108_tree(root, [4, 2, 3])
    common = ["--data", root, "--synthetic-weights", "--skip", "3", "--trimap", "narrow"]
    runs = {}
    for tag, extra in (("plain", []), ("all", ["--all-metrics"]), ("all_b2", ["--all-metrics", "--batch", "2"])):
        j = os.path.join(str(tmp_path), tag + ".json")
        s = eval_cli.main(common + ["--out", os.path.join(str(tmp_path), tag), "--summary-json", j] + extra)
        runs[tag] = (s, json.load(open(j)))
    plain, full = runs["plain"][1]["gt_metrics"], runs["all"][1]["gt_metrics"]
    assert set(plain) == {"frames", "sad", "mse", "mse_mean", "dtssd_mean", "dtssd_norm_mean", "dtssd_sum_err2", "dtssd_mask_sum"}
    assert set(full) == set(plain) | {"grad_mean", "conn_mean", "ssda_mean"}
    for k in plain:
        assert full[k] == plain[k], k
    outs = runs["all"][0]["outputs"].values()
    frames = sum(o["metrics"]["frames"] for o in outs)
    assert frames == 9
    for k in ("grad", "conn"):
        mean = sum(o["metrics"][k + "_sum"] for o in outs) / frames
        assert abs(full[k + "_mean"] - mean) <= 1e-12 * abs(mean), k
        assert full[k + "_mean"] > 0
    ssda = sum(sum(o["metrics"]["ssda_per_frame"]) for o in outs) / frames
    assert abs(full["ssda_mean"] - ssda) <= 1e-12 * ssda
    b2 = runs["all_b2"][1]["gt_metrics"]
    for k in ("grad_mean", "conn_mean", "ssda_mean", "sad", "mse_mean", "dtssd_mean"):
        assert abs(b2[k] - full[k]) <= 1e-12 * max(1.0, abs(full[k])), k
