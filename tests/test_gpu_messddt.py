"""Farneback flow and MESSDdt on the device (otvm_optflow_farneback / otvm_matting_messddt, csrc/optflow_farneback.hip)
against the float64 restatement (tests/farneback_ref.py) and the reference's values (tests/golden/metrics_messddt.npz), and
the layers above it (ClipMetrics, run_video_matte / run_video_matte_batch, run_sharded, eval_cli --messddt).

Flow tolerance: tol = 3 x max|f32 - f64|, floored at 1e-4 px, where f32 / f64 are the restatement in float32 (OpenCV's
arithmetic) and in float64 on the same input.  The device is a second float32 evaluation, so its distance to f64 is of the
size of f32's; the factor 3 leaves room for another summation order and no more."""
import json
import os

import numpy as np
import pytest
import torch

from tests import farneback_ref as F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_messddt.npz")
AMBIGUOUS_CAP = 0.005


def _lib():
    from otvm_amd import lib as L
    return L, L.load()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def device_flow(prev, nxt):
    L, lib = _lib()
    H, W = prev.shape
    flow = torch.full((H, W, 2), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.otvm_optflow_farneback_ws_bytes(H, W), dtype=torch.uint8, device="cuda")
    dp, dn = _dev(prev), _dev(nxt)
    L.check(lib.otvm_optflow_farneback(dp.data_ptr(), dn.data_ptr(), H, W, flow.data_ptr(), ws.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "optflow_farneback")
    torch.cuda.synchronize()
    return flow.cpu().numpy()


def device_messddt(p0, t0, m0, p1, t1, m1):
    """(error, num, flow) of one pair through the C ABI."""
    L, lib = _lib()
    H, W = t0.shape
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    flow = torch.full((H, W, 2), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.otvm_optflow_farneback_ws_bytes(H, W), dtype=torch.uint8, device="cuda")
    d = [_dev(a) for a in (p0, t0, m0, p1, t1, m1)]
    ptr = lambda x: 0 if x is None else x.data_ptr()
    L.check(lib.otvm_matting_messddt(*[ptr(x) for x in d], H, W, acc.data_ptr(), flow.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "matting_messddt")
    torch.cuda.synchronize()
    a = acc.cpu().tolist()
    return a[0] / 255.0 ** 2, a[1] + 1.0, flow.cpu().numpy()


def blob_pair(seed, H, W, shift, nblobs=3):
    """Soft-edged elliptic blobs moved by `shift` (dy, dx) plus a per-blob jitter, with some deformation."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    out = [np.zeros((H, W)), np.zeros((H, W))]
    for _ in range(nblobs):
        cy, cx = rng.uniform(0.25, 0.75) * H, rng.uniform(0.25, 0.75) * W
        ry, rx = rng.uniform(0.1, 0.2) * H, rng.uniform(0.1, 0.2) * W
        edge = min(rng.uniform(0.02, 0.05) * min(H, W), 12.0 * max(1.0, min(H, W) / 1080))   # soft edges, 12 px wide at most
        #                                                                                  per 1080 rows
        jy, jx = rng.uniform(-0.5, 0.5, 2)
        for f, (oy, ox, sy, sx) in enumerate(((0, 0, 1, 1), (shift[0] + jy, shift[1] + jx, rng.uniform(0.96, 1.04),
                                                                rng.uniform(0.96, 1.04)))):
            d = np.sqrt(((yy - cy - oy) / (ry * sy)) ** 2 + ((xx - cx - ox) / (rx * sx)) ** 2)
            out[f] = np.maximum(out[f], np.clip((1.0 - d) * min(ry, rx) / edge + 0.5, 0, 1))
    return [np.clip(np.rint(a * 255), 0, 255).astype(np.uint8) for a in out]


CASES = [  # (H, W, shift (dy, dx))
    (48, 64, (0.6, -1.3)),
    (96, 128, (2.4, 1.7)),
    (480, 832, (-3.3, 5.6)),
    (1080, 1920, (6.2, -4.7)),
    (1920, 1080, (-5.4, 3.3)),
    (2160, 3840, (8.5, 7.2)),
]


@pytest.mark.parametrize("H,W,shift", CASES, ids=["%dx%d" % (w, h) for h, w, _ in CASES])
def test_flow_against_float64_restatement(H, W, shift):
    t0, t1 = blob_pair(H * 7 + W, H, W, shift)
    f32 = F.farneback(t0, t1, np.float32).astype(np.float64)
    f64 = F.farneback(t0, t1, np.float64)
    tol = max(3 * float(np.abs(f32 - f64).max()), 1e-4)
    amb = np.abs(np.abs(f64 - np.floor(f64)) - 0.5) <= tol
    share = amb.reshape(-1, 2).mean(0)
    print("%dx%d: ambiguous share dx %.5f dy %.5f" % (W, H, share[0], share[1]))
    assert np.all(share <= AMBIGUOUS_CAP), share                  # on the restatement, before the device is looked at
    gpu = device_flow(t0, t1).astype(np.float64)
    assert np.isfinite(gpu).all()
    err = np.abs(gpu - f64)
    print("%dx%d: max|gpu-f64| %.3e  tol %.3e  max|f32-f64| %.3e  mean|gpu-f64| %.3e  mean|f32-f64| %.3e  max|flow| %.2f"
          % (W, H, err.max(), tol, np.abs(f32 - f64).max(), err.mean(), np.abs(f32 - f64).mean(), np.abs(f64).max()))
    assert err.max() <= tol
    bad = (np.rint(gpu) != np.rint(f64)) & ~amb
    assert not bad.any(), int(bad.sum())
    assert np.abs(f64).max() > 1.0                                   # the case moves something


def test_messddt_against_reference_fixture():
    """Per pair: the device's (error, num) equal the restatement's MESSDdt with the device's own rounded flow exactly, and
    the reference's float64 values to 1e-12, its float32 values within 2 |ref32 - ref64| + 1e-9."""
    fx = np.load(GOLDEN)
    for ci, name in enumerate(fx["names"]):
        p, t = fx["pred_%d" % ci], fx["target_%d" % ci]
        m = F.unknown_mask(t)
        for i in range(len(t) - 1):
            e, n, flow = device_messddt(p[i], t[i], m[i], p[i + 1], t[i + 1], m[i + 1])
            e_r, n_r = F.messddt_pair(p[i], t[i], m[i], p[i + 1], t[i + 1], m[i + 1], F.rint_flow(flow))
            assert abs(e - e_r) <= 1e-12 * abs(e_r) and n == n_r, (str(name), i, e, e_r)
            e64, n64 = float(fx["err64_%d" % ci][i]), float(fx["num64_%d" % ci][i])
            e32 = float(fx["err32_%d" % ci][i])
            assert abs(e - e64) <= 1e-12 * abs(e64) and n == n64, (str(name), i, e, e64)
            assert abs(e - e32) <= 2 * abs(e32 - e64) + 1e-9, (str(name), i, e, e32)


def test_messddt_large_and_maskless_against_restatement():
    """1080p with the default mask and a maskless call: exact against the restatement on the device's rounded flow."""
    t0, t1 = blob_pair(11, 1080, 1920, (4.4, -2.6))
    rng = np.random.Generator(np.random.PCG64(3))
    p0 = np.clip(t0.astype(np.int32) + rng.integers(-40, 41, t0.shape), 0, 255).astype(np.uint8)
    p1 = np.clip(t1.astype(np.int32) + rng.integers(-40, 41, t1.shape), 0, 255).astype(np.uint8)
    for m0, m1 in ((F.unknown_mask(t0), F.unknown_mask(t1)), (None, None)):
        e, n, flow = device_messddt(p0, t0, m0, p1, t1, m1)
        e_r, n_r = F.messddt_pair(p0, t0, m0, p1, t1, m1, F.rint_flow(flow))
        assert abs(e - e_r) <= 1e-12 * abs(e_r) and n == n_r, (e, e_r, n, n_r)


def test_flow_and_sums_bit_identical_across_calls():
    t0, t1 = blob_pair(5, 480, 832, (2.2, -3.1))
    a, b = device_flow(t0, t1), device_flow(t0, t1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    m0, m1 = F.unknown_mask(t0), F.unknown_mask(t1)
    r1 = device_messddt(t1, t0, m0, t0, t1, m1)
    r2 = device_messddt(t1, t0, m0, t0, t1, m1)
    assert r1[0] == r2[0] and r1[1] == r2[1] and np.array_equal(r1[2].view(np.uint32), r2[2].view(np.uint32))
    assert np.array_equal(r1[2].view(np.uint32), a.view(np.uint32))   # the metric's flow is otvm_optflow_farneback's


def test_flow_tiny_frames():
    """H or W of 1 .. 3 (REFLECT_101 on an axis of length 1 is index 0): finite and equal to the float32 restatement to the
    tolerance of the float64 one."""
    for H, W in ((1, 1), (1, 7), (5, 1), (3, 40), (33, 2)):
        rng = np.random.Generator(np.random.PCG64(H * 100 + W))
        t0 = rng.integers(0, 256, (H, W)).astype(np.uint8)
        t1 = np.roll(t0, 1, axis=1)
        f32 = F.farneback(t0, t1, np.float32).astype(np.float64)
        f64 = F.farneback(t0, t1, np.float64)
        tol = max(3 * float(np.abs(f32 - f64).max()), 1e-4)
        gpu = device_flow(t0, t1).astype(np.float64)
        assert np.isfinite(gpu).all() and np.abs(gpu - f64).max() <= tol, (H, W, np.abs(gpu - f64).max(), tol)


def _clip(seed, H, W, T):
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for i in range(T):
        t0, _ = blob_pair(seed, H, W, (0, 0))
        t = np.roll(t0, (2 * i, -3 * i), axis=(0, 1))
        p = np.clip(t.astype(np.int32) + rng.integers(-30, 31, t.shape), 0, 255).astype(np.uint8)
        frames.append((p, t))
    return frames


@pytest.mark.parametrize("image_metrics", [False, True])
def test_clip_metrics_flow_metrics(image_metrics):
    """ClipMetrics(flow_metrics=True): every key of the plain result is equal, the new keys are exactly the three MESSDdt
    keys, and they equal direct ABI calls on each pair."""
    from otvm_amd.video import ClipMetrics
    H, W, T = 70, 90, 4
    frames = _clip(9, H, W, T)
    plain = ClipMetrics("cuda", image_metrics=image_metrics)
    full = ClipMetrics("cuda", capacity=2, image_metrics=image_metrics, flow_metrics=True)   # (also grows the buffers)
    for p, t in frames:
        dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
        plain.add(dp, dt, "unknown")
        full.add(dp, dt, "unknown")
    a, b = plain.result(), full.result()
    for k, v in a.items():
        assert b[k] == v, k
    assert set(b) - set(a) == {"messddt_per_pair", "messddt_num_per_pair", "messddt_sum"}
    assert len(b["messddt_per_pair"]) == T - 1
    for i in range(1, T):
        (p0, t0), (p1, t1) = frames[i - 1], frames[i]
        e, n, _ = device_messddt(p0, t0, F.unknown_mask(t0), p1, t1, F.unknown_mask(t1))
        assert b["messddt_per_pair"][i - 1] == e and b["messddt_num_per_pair"][i - 1] == n, i
    assert b["messddt_sum"] == sum(b["messddt_per_pair"]) and b["messddt_sum"] > 0


def test_eval_cli_messddt(tmp_path, monkeypatch):
    """eval_cli --messddt over a small VideoMatting108 tree: messddt_mean is the mean of the per-clip pair sums; without the
    flag the summary has today's keys; with --all-metrics the other keys are unchanged; --batch 2 (run_video_matte_batch)
    gives the same per-pair values as batch 1 (run_video_matte) and the same means."""
    from otvm_amd import engine, eval_cli
    from tests.test_gpu_multirank import _v108_tree
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    root = os.path.join(str(tmp_path), "data")
    os.makedirs(root)
    _v108_tree(root, [4, 2, 3])
    common = ["--data", root, "--synthetic-weights", "--skip", "3", "--trimap", "narrow"]
    runs = {}
    for tag, extra in (("plain", []), ("all", ["--all-metrics"]), ("mess", ["--messddt"]),
                       ("all_mess", ["--all-metrics", "--messddt"]), ("mess_b2", ["--messddt", "--batch", "2"])):
        j = os.path.join(str(tmp_path), tag + ".json")
        s = eval_cli.main(common + ["--out", os.path.join(str(tmp_path), tag), "--summary-json", j] + extra)
        runs[tag] = (s, json.load(open(j)))
    plain, mess = runs["plain"][1]["gt_metrics"], runs["mess"][1]["gt_metrics"]
    assert set(plain) == {"frames", "sad", "mse", "mse_mean", "dtssd_mean", "dtssd_norm_mean", "dtssd_sum_err2", "dtssd_mask_sum"}
    assert set(mess) == set(plain) | {"messddt_mean", "messddt_norm_mean"}
    for k in plain:
        assert mess[k] == plain[k], k
    full, all_mess = runs["all"][1]["gt_metrics"], runs["all_mess"][1]["gt_metrics"]
    assert set(all_mess) == set(full) | {"messddt_mean", "messddt_norm_mean"}
    for k in full:
        assert all_mess[k] == full[k], k
    outs = runs["mess"][0]["outputs"]
    pairs = sum(len(o["metrics"]["messddt_per_pair"]) for o in outs.values())
    assert pairs == 3 + 1 + 2
    mean = sum(o["metrics"]["messddt_sum"] for o in outs.values()) / pairs
    assert abs(mess["messddt_mean"] - mean) <= 1e-12 * abs(mean) and mean > 0
    norm = sum(sum(e / n for e, n in zip(o["metrics"]["messddt_per_pair"], o["metrics"]["messddt_num_per_pair"]))
               for o in outs.values()) / pairs
    assert abs(mess["messddt_norm_mean"] - norm) <= 1e-12 * abs(norm)
    assert abs(all_mess["messddt_mean"] - mess["messddt_mean"]) <= 1e-12 * abs(mean)
    b2 = runs["mess_b2"]
    for i, o in outs.items():
        assert b2[0]["outputs"][i]["metrics"]["messddt_per_pair"] == o["metrics"]["messddt_per_pair"], i
    for k in ("messddt_mean", "messddt_norm_mean", "sad", "dtssd_mean"):
        assert abs(b2[1]["gt_metrics"][k] - mess[k]) <= 1e-12 * max(1.0, abs(mess[k])), k
