"""Time MESSDdt (otvm_matting_messddt: Farneback flow of the ground-truth pair + the transposed-lookup sums) per pair with
device events, and the CPU restatement of the flow (tests/farneback_ref.py, numpy float32 -- a labelled CPU figure, not cv2).

    python tools/messddt_bench.py [--iters 20] [--sizes 480x832,1080x1920,2160x3840] [--no-cpu] [--json out.json]
                                  [--eval-cli-frames 30]

Per size: device ms/pair of one call between two events (median of --iters), the same back to back, and the restatement's
time for one flow.  The split over the kernels comes from a kernel trace (rocprofv3 --kernel-trace --stats).
--eval-cli-frames N: frames/s of eval_cli --all-metrics over a one-clip 1080p VideoMatting108 tree of N frames, with and
without --messddt (alternating runs after an untimed one that plans the resolution).
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


def pair(rng, H, W):
    """A soft-edged ground truth, the same moved by (3, -2) px, and noisy predictions of both."""
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.standard_normal((H + 8, W + 8)).astype(np.float32), 16.0, mode="wrap")
    f = (f - f.min()) / max(1e-12, f.max() - f.min())
    a = np.clip(np.rint(f * 290 - 20), 0, 255).astype(np.uint8)
    t0, t1 = a[4:4 + H, 4:4 + W], a[6:6 + H, 1:1 + W]
    p0, p1 = (np.clip(t.astype(np.int32) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8) for t in (t0, t1))
    return [np.ascontiguousarray(x) for x in (p0, t0, p1, t1)]


def bench_device(p0, t0, p1, t1, iters):
    from otvm_amd import lib as L
    lib = L.load()
    H, W = t0.shape
    d = [torch.from_numpy(x).cuda() for x in (p0, t0, p1, t1)]
    m0, m1 = (((t > 0) & (t < 255)).to(torch.uint8) for t in (d[1], d[3]))
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.otvm_optflow_farneback_ws_bytes(H, W), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        L.check(lib.otvm_matting_messddt(d[0].data_ptr(), d[1].data_ptr(), m0.data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                         m1.data_ptr(), H, W, acc.data_ptr(), None, ws.data_ptr(), st), "matting_messddt")
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
    t0e = torch.cuda.Event(enable_timing=True); t1e = torch.cuda.Event(enable_timing=True)
    t0e.record()
    for _ in range(iters):
        call()
    t1e.record()
    torch.cuda.synchronize()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], back_to_back_ms=t0e.elapsed_time(t1e) / iters,
                ws_mib=lib.otvm_optflow_farneback_ws_bytes(H, W) / 2 ** 20)


def bench_cpu(t0, t1):
    from tests import farneback_ref as F
    s = time.perf_counter()
    F.farneback(t0, t1, np.float32)
    return (time.perf_counter() - s) * 1e3


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
    common = ["--data", root, "--out", os.path.join(root, "out"), "--synthetic-weights", "--trimap", "narrow", "--all-metrics"]
    eval_cli.main(common)                                   # plans (and times) the resolution once
    fps = {"all_metrics": [], "all_metrics_messddt": []}
    for _ in range(reps):
        fps["all_metrics"].append(eval_cli.main(common)["fps"])
        fps["all_metrics_messddt"].append(eval_cli.main(common + ["--messddt"])["fps"])
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="480x832,1080x1920,2160x3840")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--eval-cli-frames", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(3))
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        p0, t0, p1, t1 = pair(rng, H, W)
        row = dict(H=H, W=W, **bench_device(p0, t0, p1, t1, args.iters))
        if not args.no_cpu:
            row["cpu_restatement_flow_ms"] = bench_cpu(t0, t1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("| size | device ms/pair (median, events) | back-to-back ms/pair | workspace MiB | CPU restatement flow ms (numpy, not cv2) |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %dx%d | %.3f | %.3f | %.0f | %s |" % (r["W"], r["H"], r["median_ms"], r["back_to_back_ms"], r["ws_mib"],
                                                   "%.0f" % r["cpu_restatement_flow_ms"] if "cpu_restatement_flow_ms" in r else "-"))
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.eval_cli_frames:
        doc["eval_cli_1080p_fps"] = fps = bench_eval_cli(args.eval_cli_frames)
        print("eval_cli --all-metrics 1080p, %d frames: %s frames/s without --messddt, %s with" % (
            args.eval_cli_frames, ", ".join("%.2f" % x for x in fps["all_metrics"]),
            ", ".join("%.2f" % x for x in fps["all_metrics_messddt"])))
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
