"""Time working-resolution matting with device events:

    python tools/guided_bench.py [--iters 30] [--cases 2160x3840x2,1080x1920x2,2160x3840x4] [--radius 2] [--channels 1,4]
                                 [--clip-frames 12] [--native] [--reps 2] [--skip 10] [--max-num 5] [--json out.json]

Per case (H x W x scale) and channel count: otvm_downsample_u8, otvm_guided_coeffs (both passes) and otvm_guided_apply, median of
--iters launches, each between two events, with the bytes each pass must move beside the time.
--clip-frames N: frames/s of run_video_matte on one synthetic 3840x2160 clip of N frames with work_scale=2; --native adds the same
clip without the option (the launches of the parent commit), alternating, --reps each.  Set OTVM_TUNE_FILE or OTVM_AUTOTUNE=0 so
that every run uses one set of convolution configurations."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fgr_bench import median_ms  # noqa: E402


def bench_case(H, W, s, C, r, iters):
    from otvm_amd.guided import GuidedUpsampler, downsample_u8
    dev = torch.device("cuda", 0)
    ups = GuidedUpsampler(dev, H, W, s, r, 1e-4, C)
    h, w = ups.h, ups.w
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    work = downsample_u8(frame, s)
    targets = list(torch.rand(C, h, w, device=dev))
    row = dict(H=H, W=W, s=s, C=C, r=r, h=h, w=w)
    row["reduce_us"] = 1e3 * median_ms(lambda: downsample_u8(frame, s), iters)
    row["coeffs_us"] = 1e3 * median_ms(lambda: ups.coeffs(work, targets), iters)
    row["apply_us"] = 1e3 * median_ms(lambda: ups.apply(frame), iters)
    # bytes each pass must move: reduce = the frame in, the working frame out; coeffs = working frame + targets in, raw out, raw in,
    # mean out; apply = the frame + the mean coefficients in (once: they are 1 / s^2 of the output), fp32 planes + alpha bytes out
    row["reduce_mb"] = (H * W * 3 + h * w * 3) / 1e6
    row["coeffs_mb"] = (h * w * (3 + 4 * C) + 3 * h * w * C * 16) / 1e6
    row["apply_mb"] = (H * W * 3 + h * w * C * 16 + H * W * (4 * C + 1)) / 1e6
    for k in ("reduce", "coeffs", "apply"):
        row[k + "_gbps"] = row[k + "_mb"] / row[k + "_us"] * 1e3
    return row


def bench_clip(frames, reps, native, skip, max_num):
    from otvm_amd import helpers
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    H, W = 2160, 3840
    clip, tri = synthetic_clip(H, W, frames, seed=7)
    dclip = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in clip]
    kws = dict(work2=dict(work_scale=2))
    if native:
        kws["native"] = {}
    common = dict(trimap=tri, keep_on_device=True, skip=skip, max_num=max_num)
    for k in kws:                                              # plans (and times) each form once, untimed
        run_video_matte(m, dclip[:3], **common, **kws[k])
    fps = {k: [] for k in kws}
    for _ in range(reps):
        for k in kws:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_video_matte(m, dclip, **common, **kws[k])
            torch.cuda.synchronize()
            fps[k].append(frames / (time.perf_counter() - t0))
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--cases", default="2160x3840x2,1080x1920x2,2160x3840x4")
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--channels", default="1,4")
    ap.add_argument("--clip-frames", type=int, default=0)
    ap.add_argument("--native", action="store_true")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-num", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for case in args.cases.split(","):
        H, W, s = (int(v) for v in case.split("x"))
        for C in (int(v) for v in args.channels.split(",")):
            rows.append(bench_case(H, W, s, C, args.radius, args.iters))
            print(json.dumps(rows[-1]), flush=True)
    print("| size | s | C | reduce us (MB, GB/s) | coeffs us (MB, GB/s) | apply us (MB, GB/s) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %dx%d | %d | %d | %.1f (%.1f, %.0f) | %.1f (%.1f, %.0f) | %.1f (%.1f, %.0f) |" % (
            r["W"], r["H"], r["s"], r["C"], r["reduce_us"], r["reduce_mb"], r["reduce_gbps"], r["coeffs_us"], r["coeffs_mb"],
            r["coeffs_gbps"], r["apply_us"], r["apply_mb"], r["apply_gbps"]))
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        doc["clip_4k_fps"] = fps = bench_clip(args.clip_frames, args.reps, args.native, args.skip, args.max_num)
        print("run_video_matte 3840x2160, %d frames, skip %d, max_num %d: %s" % (
            args.clip_frames, args.skip, args.max_num,
            " | ".join("%s %s frames/s" % (k, ", ".join("%.2f" % v for v in vs)) for k, vs in fps.items())))
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
