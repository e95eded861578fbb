"""Time multi-subject matting with device events and write the report:

    python tools/subjects_bench.py [--iters 30] [--counts 1,2,4] [--clip-frames 48] [--reps 3] [--md profiles/subjects_bench.md]

Per launch at 1920x1080 with 512x640 windows, for S subjects: each of otvm_subjects_track / _crop / _bbox / _resolve beside S calls
of its single-subject counterpart (otvm_roi_track, otvm_roi_crop_at, otvm_trimap_bbox, otvm_roi_paste_at), median of --iters,
each between two events.  Per clip: subject-frames/s of run_video_matte_subjects(roi=("track", 512, 640)) beside S sequential
run_video_matte(trimap=..., roi=("track", 512, 640)) runs of the same clip, alternating, --reps each, in ONE process and with one
OTVM_TUNE_FILE (the tool sets a temporary one when none is given)."""
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

H, W = 1080, 1920
SIZE = (WIN_H, WIN_W)
CENTRES = ((540, 400), (540, 1520), (520, 800), (560, 1120))        # the windows of the last two overlap each other and their neighbours


def subject_mask(cy, cx):
    """roi_bench's soft ellipse at (cy, cx)"""
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.sqrt(((yy - cy) / RY) ** 2 + ((xx - cx) / RX) ** 2)
    return np.floor(np.clip((1.0 - r) * RY / 6.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)


def bench_kernels(S, iters):
    from otvm_amd import roi, subjects
    dev = torch.device("cuda", 0)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    log = torch.zeros((S, 3, 10), dtype=torch.int32, device=dev)
    for s in range(S):
        log[s, :, :8] = torch.tensor([40, 50, 470, 600, 40, 50, 470, 600], dtype=torch.int32)
        log[s, :, 8] = (H - WIN_H) // 2 + 1
        log[s, :, 9] = min(W - WIN_W, 31 + 300 * s)
    alphas = [torch.rand(SIZE, device=dev) for _ in range(S)]
    tris = [torch.rand((3,) + SIZE, device=dev) for _ in range(S)]
    fgrs = [torch.rand((3,) + SIZE, device=dev) for _ in range(S)]
    us = lambda fn: 1e3 * median_ms(fn, iters)
    some = ("alpha", "alpha_u8", "trimap")
    each = lambda fn: (lambda: [fn(s) for s in range(S)])
    row = dict(S=S)
    row["track_us"] = us(lambda: subjects.track(log[:, 0, :8], log[:, 0, 8:], log[:, 1, 8:], SIZE, H, W, 16))
    row["track_single_us"] = us(each(lambda s: roi.track(log[s, 0, :8], log[s, 0, 8:], log[s, 2, 8:], SIZE, H, W, 16)))
    row["crop_us"] = us(lambda: subjects.crop(log[:, 1, 8:], SIZE, frame=frame))
    row["crop_single_us"] = us(each(lambda s: roi.crop_at(log[s, 1, 8:], SIZE, frame=frame)))
    row["bbox_us"] = us(lambda: subjects.bbox(tris, log[:, 2, :8]))
    row["bbox_single_us"] = us(each(lambda s: roi.trimap_bbox(tris[s], log[s, 2, :8])))
    row["resolve_us"] = us(lambda: subjects.resolve(log[:, 1, 8:], SIZE, H, W, alphas, tris))
    row["resolve_normalise_us"] = us(lambda: subjects.resolve(log[:, 1, 8:], SIZE, H, W, alphas, tris, normalise=True))
    row["paste_single_us"] = us(each(lambda s: roi.paste_at(log[s, 1, 8:], SIZE, H, W, alphas[s], tris[s], want=some)))
    row["resolve_fgr_us"] = us(lambda: subjects.resolve(log[:, 1, 8:], SIZE, H, W, alphas, tris, fgrs, frame,
                                                        want=some + ("fgr", "union", "union_u8", "owner")))
    row["paste_fgr_single_us"] = us(each(lambda s: roi.paste_at(log[s, 1, 8:], SIZE, H, W, alphas[s], tris[s], fgrs[s], frame)))
    return row


def bench_clips(counts, frames, reps):
    from otvm_amd import helpers
    from otvm_amd.masks import trimap_from_mask
    from otvm_amd.subjects import run_video_matte_subjects
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    clip, _ = synthetic_clip(H, W, frames, seed=7)
    dclip = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in clip]
    tris = [trimap_from_mask(torch.from_numpy(subject_mask(cy, cx)).cuda(), 12).cpu().numpy() for cy, cx in CENTRES[:max(counts)]]
    roi_spec = ("track",) + SIZE
    out = {}
    for S in counts:
        routes = {"lockstep": lambda n, S=S: run_video_matte_subjects(m, dclip[:n], tris[:S], roi=roi_spec, keep_on_device=True),
                  "sequential": lambda n, S=S: [run_video_matte(m, dclip[:n], trimap=tris[s], roi=roi_spec, keep_on_device=True)
                                                for s in range(S)]}
        for k in routes:                                       # plans (and times) each form once, untimed
            routes[k](min(frames, 3))
        fps = {k: [] for k in routes}
        for _ in range(reps):
            for k in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                routes[k](frames)
                torch.cuda.synchronize()
                fps[k].append(S * frames / (time.perf_counter() - t0))
        out[S] = fps
        print("S = %d: %s" % (S, " | ".join("%s %s subject-frames/s" % (k, ", ".join("%.2f" % v for v in vs)) for k, vs in fps.items())),
              flush=True)
        m.drop_plans()                                         # every (size, S) is a plan of its own
    return out


def report(doc, args):
    L = ["# Multi-subject matting: measured launch times, S subjects in lock-step beside S sequential runs", "",
         "`tools/subjects_bench.py`; kernels in `otvm_amd/csrc/subjects.hip` (`-ffp-contract=off`).  No number here is an acceptance",
         "bar: nothing had been measured before this run, and no threshold was fixed in advance.", "",
         "## Per launch", "",
         "Device: %s.  `python tools/subjects_bench.py --iters %d --counts %s --clip-frames %d --reps %d`.  Median of %d calls" % (
             doc["device"], args.iters, args.counts, args.clip_frames, args.reps, args.iters),
         "through `otvm_amd/subjects.py` / `otvm_amd/roi.py` (the launch and the allocation of the fresh outputs), each between two",
         "device events, three untimed calls first.  Frame 1920x1080, windows %dx%d.  Each cell: the one launch over S subjects / S" % (WIN_W, WIN_H),
         "calls of the single-subject kernel (`otvm_roi_track`, `otvm_roi_crop_at` of the frame, `otvm_trimap_bbox`, `otvm_roi_paste_at`).",
         "The resolve also writes the union, its byte and the owner map, which the S pastes do not.", "",
         "| S | track us | crop frame us | bbox us | resolve (alpha, u8, trimap, union, union u8, owner) / S pastes (alpha, u8, trimap) us "
         "| the same with `normalise` us | with F / S pastes with F us |",
         "|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        L.append("| %d | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.1f | %.1f / %.1f |" % (
            r["S"], r["track_us"], r["track_single_us"], r["crop_us"], r["crop_single_us"], r["bbox_us"], r["bbox_single_us"],
            r["resolve_us"], r["paste_single_us"], r["resolve_normalise_us"], r["resolve_fgr_us"], r["paste_fgr_single_us"]))
    if doc.get("clips"):
        L += ["", "## S subjects of one clip: lock-step beside S sequential runs", "",
              "Same run, same process, same device, one `OTVM_TUNE_FILE`: one synthetic 1920x1080 clip of %d device-resident uint8" % args.clip_frames,
              "frames and S first-frame trimaps (soft ellipses of half-axes 205 x 268, band 12, side by side; the windows of neighbours",
              "overlap).  Lock-step: `run_video_matte_subjects(roi=(\"track\", %d, %d))`.  Sequential: S calls of" % SIZE,
              "`run_video_matte(trimap=..., roi=(\"track\", %d, %d))`.  Each route planned on three untimed frames first, then the two" % SIZE,
              "alternating, %d repetitions, a host clock around the route ending in a device synchronise.  Subject-frames/s = S x frames / seconds." % args.reps, "",
              "| S | lock-step subject-frames/s | sequential subject-frames/s | ratio of the medians |", "|---|---|---|---|"]
        for S, fps in sorted(doc["clips"].items(), key=lambda kv: int(kv[0])):
            L.append("| %d | %s | %s | %.2f |" % (int(S), ", ".join("%.2f" % v for v in fps["lockstep"]),
                                                 ", ".join("%.2f" % v for v in fps["sequential"]),
                                                 float(np.median(fps["lockstep"]) / np.median(fps["sequential"]))))
        L += ["", "What this does and does not show: the rate of the two routes on one box.  The weights are synthetic, so the windows",
              "follow noise and stay where the first frame put them; the lock-step route also writes a union and an owner map per",
              "frame, which the sequential runs do not.  Nothing is said about matting quality."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--counts", default="1,2,4")
    ap.add_argument("--clip-frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "subjects_bench.md"))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not os.environ.get("OTVM_TUNE_FILE"):
        os.environ["OTVM_TUNE_FILE"] = os.path.join(tempfile.mkdtemp(), "tune.json")
    counts = [int(v) for v in args.counts.split(",")]
    rows = []
    for S in counts:
        rows.append(bench_kernels(S, args.iters))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        doc["clips"] = bench_clips(counts, args.clip_frames, args.reps)
    text = report(doc, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
