"""Time region-of-interest matting with device events and write the report:

    python tools/roi_bench.py [--iters 30] [--clip-frames 24] [--reps 3] [--md profiles/roi_bench.md] [--json out.json]

The three kernels alone at 1920x1080 and 3840x2160 (otvm_trimap_bbox on a float trimap and on a label map, otvm_roi_crop and
otvm_roi_paste of a 512x640 window; median of --iters calls, each between two events), the pre-pass per mask (conversion + box),
and frames/s of run_video_matte on one synthetic 1920x1080 ``masks=`` clip of --clip-frames frames whose moving subject fits a
512x640 window, with and without roi="auto", alternating, --reps each, in ONE process and with one OTVM_TUNE_FILE (the tool sets a
temporary one when none is given), so that both routes launch one set of convolution configurations."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fgr_bench import median_ms  # noqa: E402

WIN_H, WIN_W = 512, 640


RY, RX = 205, 268       # the subject's half-axes: with band 12 and margin 32 its unknown box needs 480 < h <= 512, 608 < w <= 640


def subject_mask(H, W, t):
    """A soft ellipse (half-axes RY, RX) that moves (2, 4) pixels a frame"""
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.sqrt(((yy - H / 2 - 2.0 * t) / RY) ** 2 + ((xx - W / 2 - 4.0 * t) / RX) ** 2)
    return np.floor(np.clip((1.0 - r) * RY / 6.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)


def bench_kernels(H, W, iters):
    from otvm_amd import roi
    from otvm_amd.masks import trimap_from_mask
    dev = torch.device("cuda", 0)
    mask = torch.from_numpy(subject_mask(H, W, 0)).to(dev)
    tri = trimap_from_mask(mask, 12)
    lab = trimap_from_mask(mask, 12, labels=True)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    win = ((H - WIN_H) // 2 + 1, (W - WIN_W) // 2 + 1, WIN_H, WIN_W)
    out = torch.empty(8, dtype=torch.int32, device=dev)
    w_alpha = torch.rand((WIN_H, WIN_W), device=dev)
    w_tri, w_fgr = torch.rand((3, WIN_H, WIN_W), device=dev), torch.rand((3, WIN_H, WIN_W), device=dev)
    us = lambda fn: 1e3 * median_ms(fn, iters)
    row = dict(H=H, W=W)
    row["bbox_trimap_us"] = us(lambda: roi.trimap_bbox(tri, out))
    row["bbox_labels_us"] = us(lambda: roi.trimap_bbox(lab, out))
    row["crop_frame_us"] = us(lambda: roi.crop(win, frame=frame))
    row["crop_frame_trimap_us"] = us(lambda: roi.crop(win, frame=frame, trimap=tri))
    row["paste_alpha_us"] = us(lambda: roi.paste(win, H, W, w_alpha, w_tri, want=("alpha", "alpha_u8", "trimap")))
    row["paste_alpha_outside_us"] = us(lambda: roi.paste(win, H, W, w_alpha, w_tri, outside=tri, want=("alpha", "alpha_u8", "trimap")))
    row["paste_all_us"] = us(lambda: roi.paste(win, H, W, w_alpha, w_tri, w_fgr, frame, outside=tri))
    row["prepass_per_mask_us"] = us(lambda: roi.trimap_bbox(trimap_from_mask(mask, 12), out))
    # bytes the passes must move: the three planes in (box); 17 bytes per pixel out, the window's 16 in (paste without F and
    # outside); with everything 29 out, 15 in per frame pixel and 28 in per window pixel
    row["bbox_trimap_gbps"] = 12 * H * W / row["bbox_trimap_us"] / 1e3
    row["paste_alpha_gbps"] = (17 * H * W + 16 * WIN_H * WIN_W) / row["paste_alpha_us"] / 1e3
    row["paste_all_gbps"] = (44 * H * W + 28 * WIN_H * WIN_W) / row["paste_all_us"] / 1e3
    return row


def bench_clip(frames, reps, margin):
    from otvm_amd import helpers
    from otvm_amd.masks import Mask
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    H, W = 1080, 1920
    clip, _ = synthetic_clip(H, W, frames, seed=7)
    dclip = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in clip]
    masks = [Mask(torch.from_numpy(subject_mask(H, W, t)).cuda(), band=12) for t in range(frames)]
    common = dict(keep_on_device=True)
    routes = {"roi": lambda n: run_video_matte(m, dclip[:n], masks=masks[:n], roi="auto", roi_margin=margin, **common),
              "full": lambda n: run_video_matte(m, dclip[:n], masks=masks[:n], **common)}
    size = None
    for k in routes:                                           # plans (and times) each form once, untimed
        size = routes[k](min(frames, 3)).get("roi_size", size)
    fps = {k: [] for k in routes}
    for _ in range(reps):
        for k in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k](frames)
            torch.cuda.synchronize()
            fps[k].append(frames / (time.perf_counter() - t0))
    return fps, size


def report(doc, args):
    L = ["# Region-of-interest matting: measured kernel times, the `masks=` route with and without a window", "",
         "`tools/roi_bench.py`; kernels in `otvm_amd/csrc/roi.hip` (`-ffp-contract=off`).  No speed number here is an acceptance bar:",
         "nothing had been measured before this run, and no threshold was fixed in advance.", "",
         "## The kernels alone", "",
         "Device: %s.  `python tools/roi_bench.py --iters %d --clip-frames %d --reps %d`.  Median of %d calls through" % (
             doc["device"], args.iters, args.clip_frames, args.reps, args.iters),
         "`otvm_amd/roi.py` (the launch and the allocation of the fresh outputs), each between two device events, three untimed calls",
         "first.  The window is %dx%d at an odd origin; the trimap is that of a soft ellipse of half-axes 205 x 268, band 12.  The calls" % (WIN_W, WIN_H),
         "repeat over buffers that fit the 256 MB last-level cache, so the rates are not HBM rates.", "",
         "| frame | box, float trimap us (GB/s) | box, labels us | crop frame us | crop frame + trimap us | paste alpha, u8, trimap us (GB/s) "
         "| the same with `outside` us | paste with F and `outside` us (GB/s) | pre-pass per mask us |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        L.append("| %dx%d | %.1f (%.0f) | %.1f | %.1f | %.1f | %.1f (%.0f) | %.1f | %.1f (%.0f) | %.1f |" % (
            r["W"], r["H"], r["bbox_trimap_us"], r["bbox_trimap_gbps"], r["bbox_labels_us"], r["crop_frame_us"], r["crop_frame_trimap_us"],
            r["paste_alpha_us"], r["paste_alpha_gbps"], r["paste_alpha_outside_us"], r["paste_all_us"], r["paste_all_gbps"],
            r["prepass_per_mask_us"]))
    L += ["", "The pre-pass per mask is `otvm_trimap_from_mask` (two launches) and `otvm_trimap_bbox` (two launches) on a mask that is",
          "already on the device; a clip pays it once per frame before the first frame runs, and reads all boxes back with one copy."]
    if doc.get("clip_fps"):
        fps = doc["clip_fps"]
        L += ["", "## `masks=` with and without `roi=\"auto\"`", "",
              "Same run, same process, same device, one `OTVM_TUNE_FILE`: one synthetic 1920x1080 clip of %d device-resident uint8" % args.clip_frames,
              "frames with a mask per frame (a soft ellipse of half-axes 205 x 268 that moves (2, 4) pixels a frame, band 12, `roi_margin` %d);" % args.margin,
              "each route planned on three untimed frames first, then the two routes alternating, %d repetitions, a host clock around" % args.reps,
              "`run_video_matte` ending in a device synchronise.  The window `roi=\"auto\"` chose is %s (h x w).  The timed call of the" % (
                  "%dx%d" % tuple(doc["clip_roi_size"]) if doc.get("clip_roi_size") else "?"),
              "`roi` route includes its pre-pass (every mask converted once more, one read-back).", "",
              "| route | frames/s |", "|---|---|",
              "| `run_video_matte(masks=[...], roi=\"auto\")` | %s |" % ", ".join("%.2f" % v for v in fps["roi"]),
              "| `run_video_matte(masks=[...])` (the full frame) | %s |" % ", ".join("%.2f" % v for v in fps["full"]), "",
              "The two routes do not compute the same matte: the window's result is the matte of the cropped clip pasted back (the",
              "decoder's pyramid pooling sees the window, not the frame).  With no trained checkpoint here nothing is said about how",
              "the two compare on real footage."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--clip-frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--margin", type=int, default=32)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "roi_bench.md"))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    tmp = None
    if not os.environ.get("OTVM_TUNE_FILE"):
        tmp = tempfile.mkdtemp()
        os.environ["OTVM_TUNE_FILE"] = os.path.join(tmp, "tune.json")
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        rows.append(bench_kernels(H, W, args.iters))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        fps, size = bench_clip(args.clip_frames, args.reps, args.margin)
        doc["clip_fps"], doc["clip_roi_size"] = fps, list(size) if size else None
        print("run_video_matte 1920x1080 masks=, %d frames, alternating: %s | window %s" % (
            args.clip_frames, " | ".join("%s %s frames/s" % (k, ", ".join("%.2f" % v for v in vs)) for k, vs in fps.items()), size), flush=True)
    text = report(doc, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
