"""Time trimaps from masks with device events:

    python tools/mask_trimap_bench.py [--iters 30] [--sizes 480x832,1080x1920,2160x3840] [--radii 5,12,20]
                                      [--clip-frames 24] [--reps 3] [--skip 10] [--max-num 5] [--json out.json]

Per size (H x W) and band radius: otvm_trimap_from_mask (both launches) writing the one-hot planes, median of --iters launches,
each between two events, on a soft blob mask and on a disc (a deep interior: the longest scans of the row pass); beside the time
the bytes the two passes must move.
--clip-frames N: frames/s of run_video_matte on one synthetic 1920x1080 clip of N frames through ``masks=`` (every frame from its
own mask, nothing propagated) and through ``trimap=`` (the first frame's trimap propagated), alternating, --reps each, one
process; with the launches per frame of either route (the engine's launch lists plus what the route adds).  Set OTVM_TUNE_FILE or
OTVM_AUTOTUNE=0 so that every run uses one set of convolution configurations."""
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


def blob_mask(H, W, seed=0):
    g = np.random.default_rng(seed)
    cell = max(8, H // 12)
    m = np.kron(g.random((H // cell + 2, W // cell + 2)), np.ones((cell, cell)))[:H, :W]
    return np.where(m > 0.6, 255, np.where(m < 0.4, 0, (255 * g.random((H, W))))).astype(np.uint8)


def disc_mask(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (H / 3) ** 2, 255, 0).astype(np.uint8)


def bench_call(H, W, r, iters):
    from otvm_amd.masks import MaskTrimapper, band_thresholds
    dev = torch.device("cuda", 0)
    tm = MaskTrimapper(dev, H, W)
    t_fg, t_bg = band_thresholds(r)
    row = dict(H=H, W=W, r=r)
    for name, m in (("blob", blob_mask(H, W)), ("disc", disc_mask(H, W))):
        md = torch.from_numpy(m).to(dev)
        row[name + "_us"] = 1e3 * median_ms(lambda: tm(md, t_fg, t_bg, 127, 128), iters)
        row[name + "_labels_us"] = 1e3 * median_ms(lambda: tm(md, t_fg, t_bg, 127, 128, labels=True, band_label=255), iters)
    # bytes the passes must move: the mask in and 2 bytes per pixel out (columns); those 2 bytes in and three fp32 planes out (rows)
    row["mb"] = H * W * (1 + 2 + 2 + 12) / 1e6
    row["blob_gbps"] = row["mb"] / row["blob_us"] * 1e3
    return row


def bench_clip(frames, reps, skip, max_num):
    from otvm_amd import helpers
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    H, W = 1080, 1920
    clip, tri = synthetic_clip(H, W, frames, seed=7)
    dclip = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in clip]
    yy, xx = np.mgrid[0:H, 0:W]
    dmasks = []
    for t in range(frames):                                    # the clip's moving disc, a soft rim
        r = np.sqrt((yy - H / 2 - 0.5 * t) ** 2 + (xx - W / 2 - 1.0 * t) ** 2)
        dmasks.append(torch.from_numpy(np.floor(np.clip((H / 4 - r) / 6.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)).cuda())
    common = dict(keep_on_device=True, skip=skip, max_num=max_num)
    routes = dict(masks=lambda n: run_video_matte(m, dclip[:n], masks=dmasks[:n], **common),
                  trimap=lambda n: run_video_matte(m, dclip[:n], trimap=tri, **common))
    for k in routes:                                           # plans (and times) each form once, untimed
        routes[k](min(frames, 3))
    fps = {k: [] for k in routes}
    for _ in range(reps):
        for k in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k](frames)
            torch.cuda.synchronize()
            fps[k].append(frames / (time.perf_counter() - t0))
    return fps, launches_per_frame(m, H, W)


def launches_per_frame(model, H, W):
    """Steps of the plan's launch lists.  A frame of the masks route runs "fba" and one "fba_tail" (as a first frame does) plus
    the two launches of otvm_trimap_from_mask; a later frame of the propagated route runs those two lists and the STM lists
    "segment_a", "segment_skip", "segment_b" (query encoder, memory read, decoder) and, for the frame before it, one "mem_stem"
    and "mem_trunk" (Encoder_M).  The glue launches outside the lists (preprocess, trimap encoding, crop) are common to both."""
    pl = model._engine.plan(H, W, 1)
    return {k: len(v) for k, v in sorted(pl.steps.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", default="480x832,1080x1920,2160x3840")
    ap.add_argument("--radii", default="5,12,20")
    ap.add_argument("--clip-frames", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-num", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        for r in (float(v) for v in args.radii.split(",")):
            rows.append(bench_call(H, W, r, args.iters))
            print(json.dumps(rows[-1]), flush=True)
    print("| size | r | blob: trimap us | blob: labels us | disc: trimap us | disc: labels us | MB moved (trimap) | GB/s (blob) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %dx%d | %g | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f |" % (r["W"], r["H"], r["r"], r["blob_us"], r["blob_labels_us"],
                                                                       r["disc_us"], r["disc_labels_us"], r["mb"], r["blob_gbps"]))
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        fps, launches = bench_clip(args.clip_frames, args.reps, args.skip, args.max_num)
        doc["clip_1080p_fps"], doc["launch_lists"] = fps, launches
        print("run_video_matte 1920x1080, %d frames, skip %d, max_num %d, alternating: %s" % (
            args.clip_frames, args.skip, args.max_num,
            " | ".join("%s %s frames/s" % (k, ", ".join("%.2f" % v for v in vs)) for k, vs in fps.items())))
        if launches is not None:
            print("launch lists of the 1080p plan (entries): %s" % json.dumps(launches))
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
