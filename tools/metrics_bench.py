"""Time the Grad + Conn metric kernel (otvm_matting_grad_conn) per frame with device events, against the CPU route of the
reference (float32 Gaussian-gradient filter + scipy 4-connected labelling of 10 thresholds, as tests/matting_metrics_ref.py).

    python tools/metrics_bench.py [--iters 20] [--cpu-iters 2] [--sizes 480x832,1080x1920,2160x3840] [--json out.json]
                                  [--eval-cli-frames 30]

Per size: device ms/frame of one call between two events (median of --iters), the same back to back, and the CPU route's
best of --cpu-iters.  The split over the kernels of one call comes from a kernel trace (rocprofv3 --kernel-trace --stats).
--eval-cli-frames N: frames/s of eval_cli over a one-clip 1080p VideoMatting108 tree of N frames, with and without
--all-metrics (alternating runs after an untimed one that plans the resolution).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def field(rng, H, W):
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.standard_normal((H, W)).astype(np.float32), 16.0, mode="wrap")
    f = (f - f.min()) / max(1e-12, f.max() - f.min())
    t = np.clip(np.rint(f * 290 - 20), 0, 255).astype(np.uint8)
    p = np.clip(t.astype(np.int32) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
    return p, t


def bench_device(p, t, iters):
    from otvm_amd import lib as L
    lib = L.load()
    H, W = p.shape
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    dm = ((dt > 0) & (dt < 255)).to(torch.uint8)
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.otvm_matting_grad_conn_ws_bytes(H, W), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        L.check(lib.otvm_matting_grad_conn(dp.data_ptr(), dt.data_ptr(), dm.data_ptr(), H, W, acc.data_ptr(), None,
                                           ws.data_ptr(), st), "matting_grad_conn")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    for i in range(iters):
        ev[2 * i].record()
        call()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
    # back-to-back throughput (launches overlap the previous call's tail)
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        call()
    t1.record()
    torch.cuda.synchronize()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], back_to_back_ms=t0.elapsed_time(t1) / iters)


def bench_cpu(p, t, iters):
    """The reference's CPU route, one thread: float32 9x9 filter (as ImageFilter) + 10 x (label + bincount)."""
    from scipy import ndimage
    from tests import matting_metrics_ref as R
    g, dg = R.grad_taps()
    hx = np.outer(g, dg).astype(np.float32)
    m = ((t > 0) & (t < 255)).astype(np.float32)
    out = {}
    for name, fn in (("grad", lambda: [ndimage.convolve(x.astype(np.float32) / np.float32(255), k, mode="nearest")
                                       for x in (p, t) for k in (hx, hx.T)]),
                     ("conn", lambda: R.conn(p, t, m))):
        best = 1e30
        for _ in range(iters):
            s = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - s)
        out[name + "_ms"] = best * 1e3
    return out


def bench_eval_cli(frames, reps=2):
    import tempfile
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.synth_data import soft_alpha, synthetic_clip
    H, W = 1080, 1920
    root = tempfile.mkdtemp(prefix="otvm_v108_")
    v = os.path.join(root, "VideoMatting108")
    fg, _ = synthetic_clip(H, W, frames, seed=7)
    bg, _ = synthetic_clip(H, W, frames, seed=8)
    corr = {}
    for t in range(frames):
        a = np.rint(soft_alpha(H, W, t) * 255).astype(np.uint8)
        k = "vid/clip_0/%05d.png" % t
        corr[k] = "bgs/%05d.jpg" % t
        os.makedirs(os.path.dirname(os.path.join(v, "FG_done", k)), exist_ok=True)
        Image.fromarray(np.concatenate([fg[t][..., ::-1], a[..., None]], -1)).save(os.path.join(v, "FG_done", k))
        os.makedirs(os.path.join(v, "BG_done2", "bgs"), exist_ok=True)
        Image.fromarray(bg[t][..., ::-1].copy()).save(os.path.join(v, "BG_done2", "bgs", "%05d.png" % t))
    json.dump(corr, open(os.path.join(v, "frame_corr.json"), "w"))
    open(os.path.join(v, "val_videos.txt"), "w").write("vid/clip_0\n")
    common = ["--data", root, "--out", os.path.join(root, "out"), "--synthetic-weights", "--trimap", "narrow"]
    eval_cli.main(common)                                   # plans (and times) the resolution once
    fps = {"plain": [], "all_metrics": []}
    for _ in range(reps):
        fps["plain"].append(eval_cli.main(common)["fps"])
        fps["all_metrics"].append(eval_cli.main(common + ["--all-metrics"])["fps"])
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-iters", type=int, default=2)
    ap.add_argument("--sizes", default="480x832,1080x1920,2160x3840")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--eval-cli-frames", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(3))
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        p, t = field(rng, H, W)
        row = dict(H=H, W=W, **bench_device(p, t, args.iters))
        if not args.no_cpu:
            row.update({"cpu_" + k: v for k, v in bench_cpu(p, t, args.cpu_iters).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("| size | device ms/frame (median, events) | back-to-back ms/frame | CPU Grad ms | CPU Conn ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %dx%d | %.3f | %.3f | %s | %s |" % (r["W"], r["H"], r["median_ms"], r["back_to_back_ms"],
                                                 "%.1f" % r["cpu_grad_ms"] if "cpu_grad_ms" in r else "-",
                                                 "%.1f" % r["cpu_conn_ms"] if "cpu_conn_ms" in r else "-"))
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.eval_cli_frames:
        doc["eval_cli_1080p_fps"] = fps = bench_eval_cli(args.eval_cli_frames)
        print("eval_cli 1080p, %d frames: %s frames/s without --all-metrics, %s with" % (
            args.eval_cli_frames, ", ".join("%.2f" % x for x in fps["plain"]), ", ".join("%.2f" % x for x in fps["all_metrics"])))
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
