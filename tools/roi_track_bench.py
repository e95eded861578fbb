"""Time the tracking window of region-of-interest matting with device events and write the report:

    python tools/roi_track_bench.py [--iters 30] [--clip-frames 24] [--reps 3] [--md profiles/roi_track_bench.md] [--json out.json]

Per launch at 1920x1080: otvm_roi_track, and otvm_roi_crop_at / otvm_roi_paste_at beside the host-origin otvm_roi_crop /
otvm_roi_paste for the same 512x640 window (median of --iters calls, each between two events).  Per clip: frames/s of
run_video_matte on one synthetic 1920x1080 ``trimap=`` clip of --clip-frames frames whose subject crosses the frame, on the full
frame, in the static window round the subject's whole path (sized by hand from the path) and with roi="track", alternating,
--reps each, in ONE process and with one OTVM_TUNE_FILE (the tool sets a temporary one when none is given)."""
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
from tools.roi_bench import RX, RY, WIN_H, WIN_W  # noqa: E402

STEP_Y, STEP_X = 2, 12      # pixels a frame: under hold = 16 of the default margin, so a window that follows is not outrun


def subject_mask(H, W, t, T):
    """roi_bench's soft ellipse, crossing the frame: (STEP_Y, STEP_X) pixels a frame, the path centred in the frame"""
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = H / 2 + STEP_Y * (t - (T - 1) / 2.0), W / 2 + STEP_X * (t - (T - 1) / 2.0)
    r = np.sqrt(((yy - cy) / RY) ** 2 + ((xx - cx) / RX) ** 2)
    return np.floor(np.clip((1.0 - r) * RY / 6.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)


def bench_kernels(H, W, iters):
    from otvm_amd import roi
    dev = torch.device("cuda", 0)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    lab = torch.randint(0, 3, (H, W), dtype=torch.uint8, device=dev)
    win = ((H - WIN_H) // 2 + 1, (W - WIN_W) // 2 + 1, WIN_H, WIN_W)
    size = (WIN_H, WIN_W)
    log = torch.tensor([[0, 0], list(win[:2]), [0, 0]], dtype=torch.int32, device=dev)
    box = torch.tensor([40, 50, 470, 600, 40, 50, 470, 600], dtype=torch.int32, device=dev)
    w_alpha = torch.rand(size, device=dev)
    w_tri, w_fgr = torch.rand((3,) + size, device=dev), torch.rand((3,) + size, device=dev)
    us = lambda fn: 1e3 * median_ms(fn, iters)
    some = ("alpha", "alpha_u8", "trimap")
    row = dict(H=H, W=W)
    row["track_us"] = us(lambda: roi.track(box, log[1], log[2], size, H, W, 16))
    row["track_centre_us"] = us(lambda: roi.track(box, None, log[2], size, H, W, 16))
    row["crop_us"] = us(lambda: roi.crop(win, frame=frame))
    row["crop_at_us"] = us(lambda: roi.crop_at(log[1], size, frame=frame))
    row["crop_labels_us"] = us(lambda: roi.crop(win, frame=frame, labels=lab))
    row["crop_at_labels_us"] = us(lambda: roi.crop_at(log[1], size, frame=frame, labels=lab))
    row["paste_us"] = us(lambda: roi.paste(win, H, W, w_alpha, w_tri, want=some))
    row["paste_at_us"] = us(lambda: roi.paste_at(log[1], size, H, W, w_alpha, w_tri, want=some))
    row["paste_fgr_us"] = us(lambda: roi.paste(win, H, W, w_alpha, w_tri, w_fgr, frame))
    row["paste_at_fgr_us"] = us(lambda: roi.paste_at(log[1], size, H, W, w_alpha, w_tri, w_fgr, frame))
    return row


def bench_clip(frames, reps, margin):
    from otvm_amd import helpers, roi
    from otvm_amd.masks import trimap_from_mask
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
    tris = [trimap_from_mask(torch.from_numpy(subject_mask(H, W, t, frames)).cuda(), 12) for t in (0, frames - 1)]
    # the static window, by hand from the path: round the union of the first and the last frame's classes, with the margin
    path = roi.union([roi.boxes_of(roi.trimap_bbox(t))[1][0] for t in tris])
    h, w = roi.window_size([path], H, W, margin)
    static = roi.window_origin(path, h, w, H, W) + (h, w)
    common = dict(keep_on_device=True, trimap=tris[0].cpu().numpy())
    routes = {"track": lambda n: run_video_matte(m, dclip[:n], roi="track", roi_margin=margin, **common),
              "static": lambda n: run_video_matte(m, dclip[:n], roi=static, **common),
              "full": lambda n: run_video_matte(m, dclip[:n], **common)}
    sizes = {}
    for k in routes:                                           # plans (and times) each form once, untimed
        sizes[k] = routes[k](min(frames, 3)).get("roi_size")
    fps = {k: [] for k in routes}
    for _ in range(reps):
        for k in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k](frames)
            torch.cuda.synchronize()
            fps[k].append(frames / (time.perf_counter() - t0))
    return fps, sizes


def report(doc, args):
    L = ["# The tracking window of region-of-interest matting: measured launch times, a `trimap=` clip three ways", "",
         "`tools/roi_track_bench.py`; kernels in `otvm_amd/csrc/roi.hip` (`-ffp-contract=off`).  No number here is an acceptance bar:",
         "nothing had been measured before this run, and no threshold was fixed in advance.", "",
         "## Per launch", "",
         "Device: %s.  `python tools/roi_track_bench.py --iters %d --clip-frames %d --reps %d`.  Median of %d calls through" % (
             doc["device"], args.iters, args.clip_frames, args.reps, args.iters),
         "`otvm_amd/roi.py` (the launch and the allocation of the fresh outputs), each between two device events, three untimed calls",
         "first.  The window is %dx%d at an odd origin; the device-origin forms (`_at`) read that origin from a row of an `int32` log," % (WIN_W, WIN_H),
         "the host-origin forms beside them are the kernels as they were, in the same run.", "",
         "| frame | `otvm_roi_track` us (with a neighbour / centring) | crop frame: host origin / `_at` us | crop frame + labels: host / `_at` us "
         "| paste alpha, u8, trimap: host / `_at` us | paste with F: host / `_at` us |",
         "|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        L.append("| %dx%d | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f |" % (
            r["W"], r["H"], r["track_us"], r["track_centre_us"], r["crop_us"], r["crop_at_us"], r["crop_labels_us"], r["crop_at_labels_us"],
            r["paste_us"], r["paste_at_us"], r["paste_fgr_us"], r["paste_at_fgr_us"]))
    if doc.get("clip_fps"):
        fps, sizes = doc["clip_fps"], doc["clip_sizes"]
        L += ["", "## A `trimap=` clip on the full frame, in a static window round the path, and with `roi=\"track\"`", "",
              "Same run, same process, same device, one `OTVM_TUNE_FILE`: one synthetic 1920x1080 clip of %d device-resident uint8" % args.clip_frames,
              "frames and the first frame's trimap (a soft ellipse of half-axes 205 x 268, band 12) whose subject crosses the frame at",
              "(%d, %d) pixels a frame; `roi_margin` %d.  The static window is sized by hand from the path (round the union of the first" % (STEP_Y, STEP_X, args.margin),
              "and the last frame's classes): %s (h x w); `roi=\"track\"` chose %s.  Each route planned on three untimed frames first, then" % (
                  "%dx%d" % tuple(sizes["static"]), "%dx%d" % tuple(sizes["track"])),
              "the three alternating, %d repetitions, a host clock around `run_video_matte` ending in a device synchronise." % args.reps, "",
              "| route | frames/s |", "|---|---|",
              "| `run_video_matte(trimap=..., roi=\"track\")` | %s |" % ", ".join("%.2f" % v for v in fps["track"]),
              "| `run_video_matte(trimap=..., roi=(y0, x0, h, w))`, the static window round the path | %s |" % ", ".join("%.2f" % v for v in fps["static"]),
              "| `run_video_matte(trimap=...)` (the full frame) | %s |" % ", ".join("%.2f" % v for v in fps["full"]), "",
              "What this does and does not show: a frame of the tracking route issues the same launches wherever its window lies",
              "(`otvm_roi_track`, one `otvm_roi_crop_at`, the network at the window's size, `otvm_trimap_bbox`, `otvm_roi_paste_at`), so",
              "the rate is that of the route.  It does NOT show a window following a subject: the weights are synthetic, the trimap they",
              "return is noise that fills the window, and a window that follows noise stays where the first frame put it.  The three",
              "routes do not compute the same matte (the decoder's pyramid pooling sees the window, not the frame), and with no trained",
              "checkpoint here nothing is said about how they compare on real footage."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", default="1080x1920")
    ap.add_argument("--clip-frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--margin", type=int, default=32)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "roi_track_bench.md"))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not os.environ.get("OTVM_TUNE_FILE"):
        os.environ["OTVM_TUNE_FILE"] = os.path.join(tempfile.mkdtemp(), "tune.json")
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        rows.append(bench_kernels(H, W, args.iters))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        fps, sizes = bench_clip(args.clip_frames, args.reps, args.margin)
        doc["clip_fps"], doc["clip_sizes"] = fps, {k: list(v) if v else None for k, v in sizes.items()}
        print("run_video_matte 1920x1080 trimap=, %d frames, alternating: %s | sizes %s" % (
            args.clip_frames, " | ".join("%s %s frames/s" % (k, ", ".join("%.2f" % v for v in vs)) for k, vs in fps.items()), sizes), flush=True)
    text = report(doc, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
