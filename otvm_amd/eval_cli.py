"""eval.py-shaped command line (reference eval.py:21-94, scripts/eval_s4_demo.sh) on the HIP path.

    python -m otvm_amd.eval_cli --demo --data ./demo --weights weights/s4_OTVM.pth --out ./demo_results [--viz]
    python -m otvm_amd.eval_cli --data <root holding VideoMatting108/> --weights weights/s4_OTVM.pth   # val split
    python -m otvm_amd.eval_cli --demo --data ./demo --synthetic-weights            # plumbing check, no checkpoint

Dataset layouts: otvm_amd/datasets.py (Demo_Test / VideoMatting108_Test, reference dataset.py:959-1070).  Without
--demo the VideoMatting108 validation split is evaluated as eval.py:86-89 does: the first-frame trimap is derived
from the ground-truth alpha with the --trimap dilation, and SAD / MSE / dtSSD against the ground truth are
accumulated on the device and reduced over ranks (--all-metrics: also Grad, Conn and SSDA).  Alpha PNGs are written as trunc(alpha*255) (eval.py:209-217);
--viz adds the six-panel composite frames (eval.py:96-115) and, when ffmpeg exists, the mp4 (eval.py:229-242).
--fgr writes the network's foreground estimate as straight-alpha RGBA PNGs, <out>/fgr/<seq>/<name>.png; --composite PATH|R,G,B
writes that foreground over a new background (an image, resized once on the host to the clip's resolution, or a colour),
<out>/comp/<seq>/<name>.png.  Both work for the demo and the VideoMatting108 layouts and with --gpus N; with --batch > 1 they
are refused (as --viz is).
--keyframes (demo layout): every trimap/<stem>.png of a clip -- not only the first frame's -- is a full keyframe and every
labels/<stem>.png (8-bit grey: 0 bg, 128 unknown, 255 fg, anything else unlabelled) a correction of the propagated trimap; the
clip is matted from the earliest trimap forward and then backward (video.keyframe_schedule), so its first frame needs no trimap.
Without the flag those files are ignored.  Frames are decoded up front in this mode; refused with --batch > 1.
--work-scale S (demo layout, S = 2, 3, 4): working-resolution matting -- the network runs on an S x S block mean of every frame and
alpha (with --fgr / --composite also the foreground) returns to the input resolution through a guided filter on the frame itself
(--work-radius R, --work-eps E: placeholders, not tuned on real footage; video.run_video_matte).  All PNGs keep the input
resolution; works with --fgr, --composite and --keyframes; refused with --viz and --batch > 1.  The summary carries work_scale and
work_size (per sequence).
--masks key|frame (demo layout): trimaps from segmentation masks, mask/<stem>.png (8-bit grey), made on the device
(otvm_amd/masks.py).  key: every mask file is a full keyframe, as a trimap file is under --keyframes; a clip needs a trimap or a
mask on at least one frame (without --keyframes only the first frame's trimap file counts).  frame: every frame needs a mask and
is matted from it alone, nothing is propagated (run_video_matte(masks=...)).  --mask-band R[,R_BG] is the reach of the unknown
band into the foreground / background in pixels (default: the --trimap dilation), --mask-thresholds LO,HI the cut (foreground
>= HI, background <= LO; default 127,128) -- placeholders, not tuned on real footage.  Works with --fgr, --composite, --work-scale
and, in key mode, --keyframes (labels/ too); refused with --batch > 1 and without --demo.  The summary carries masks, mask_band
and mask_thresholds.
--stabilise [K] (demo layout): temporal stabilisation of alpha -- a causal, flow-compensated recursive filter of strength K in
[0,1] behind every frame (video.run_video_matte(stabilise=...), otvm_amd/temporal.py); --stabilise-taus C,A sets the grey residual
and the change of alpha at which it lets go, --stabilise-region unknown|all where it acts.  The alpha PNGs, and with --fgr /
--composite the foreground bytes, carry the stabilised alpha.  The defaults (0.5; 24,0.5) are PLACEHOLDERS: there is no trained
checkpoint here, the filter is checked by definition and by property on synthetic clips, not by quality on real footage.  Works
with --masks, --keyframes (forward-only schedules), --work-scale, --fgr and --composite; refused with --viz, --batch > 1 and
without --demo.  The summary carries stabilise.
--roi auto|track[,H,W]|Y0,X0,H,W [--roi-margin M] (demo layout): region-of-interest matting -- the network runs in a window round the subject
and alpha (with --fgr / --composite also the foreground) is pasted back into the frame (video.run_video_matte(roi=...),
otvm_amd/roi.py).  auto with --masks frame tracks the mask's unknown band frame by frame; auto otherwise places ONE window round
the classes other than background of the clip's trimaps / masks / label maps, which the subject must not leave (roi_clipped in the
summary lists the frames whose propagated trimap reaches a side of the window).  The result is the matte of the cropped clip, NOT
the full-frame matte (the network's global context is the window's), it is checked by definition only, and the default margin
(32) is a PLACEHOLDER.  Works with --masks, --keyframes, --fgr, --composite and --stabilise; refused with --work-scale, --viz,
--batch > 1 and without --demo.  The summary carries roi, roi_margin and per clip roi_size and roi_clipped.  Between clips whose
window size differs the engine's frame plans are dropped (nothing else evicts them).
--roi track[,H,W] (trimap / --masks key / --keyframes clips): the TRACKING window -- one size for the clip (H,W, or the largest
source's box plus the margin), an origin per frame that lives on the device and follows the box of the trimap the network put out
for the neighbouring frame (otvm_roi_track; roi.track_origin is the policy), so the window lags ONE frame: a subject that moves more
than max(1, margin // 2) pixels a frame, or outgrows the size, is cut, and roi_clipped lists those frames.  Nothing is read back
inside the frame loop.  The same exclusions as --roi auto, and refused with --masks frame (auto tracks there).
--subjects [--subjects-overlap keep|normalise] (demo layout): one matte per subject of a clip (subjects.run_video_matte_subjects).
Every sub-directory of <seq>/subjects/ (beside trimap/) is one subject, in sorted order; its trimap is the PNG carrying the first
frame's stem, decoded as trimap/ is.  With --roi track[,H,W] every subject is followed by a tracking window of its own, all of one
size, and the windows run as one lock-step batch; without --roi the subjects run at full frames.  Per-subject alphas go to
<out>/.../pred/<seq>/<subject>/, their union (min(sum, 1)) to <out>/.../pred/<seq>/, with --fgr the RGBA to
<out>/fgr/<seq>/<subject>/.  normalise divides the alphas of a pixel by their sum where it exceeds 1 (an untuned PLACEHOLDER).
Checked by definition only.  Refused without --demo, with --roi auto or a static window, --keyframes, --masks, --work-scale,
--stabilise, --viz, --composite and --batch > 1.  The summary carries subjects and subjects_overlap; between clips whose window
size or number of subjects differs the engine's frame plans are dropped.
--key green|blue|R,G,B [--key-thresholds LO,HI] | --plate PATH [--plate-thresholds LO,HI] [--plate-radius R] (demo layout):
trimap-free matting of keyed footage (video.run_video_matte(key=...), otvm_amd/keys.py).  No trimap/ or mask/ folder is read: every
frame's mask is made on the device from the frame itself -- a hue-cone chroma key round the screen's colour, or the difference to a
clean plate of the empty set (an image of the frames' resolution) -- made into a trimap as a mask is (--mask-band and
--mask-thresholds apply), and the frame is matted from it alone; nothing is propagated.  Every default is a PLACEHOLDER, the keys
are checked by definition only, and nothing is claimed about quality on real footage.  Works with --fgr, --composite, --work-scale,
--stabilise and --roi auto|Y0,X0,H,W; --key and --plate exclude each other, --masks, --keyframes, --subjects, --roi track and
--batch > 1, and are refused without --demo.  The summary carries key.
Frame IO runs through otvm_amd/io_pipeline.py: the demo flow decodes ahead in a thread pool and uploads on a copy
stream, both flows download the 8-bit alphas asynchronously and PNG-encode them in a pool (the reference's loop blocks
on .cpu() + cv2.imwrite per frame, eval.py:209-217).
Reproducibility: the first call per resolution times the convolution configurations on the device (a per-process choice
among kernels that differ in fp32 summation order): two runs agree bit for bit only with fixed configurations -- set
OTVM_TUNE_FILE=path (choices are written once and re-used; multi-rank runs share rank 0's choices in any case) or
OTVM_AUTOTUNE=0 (built-in heuristic).  `--batch B` steps B sequences of equal resolution per launch.
Multi-GPU: `--gpus N` starts N ranks (one process per GPU) itself, or launch with torchrun; sequences are sharded
one-per-GPU and the metric sums meet in one all-reduce.
"""
import argparse
import os

import torch


def parse_composite(spec):
    """--composite: "R,G,B" (0..255) -> ((r, g, b), None); anything else is the path of an image -> (None, path)."""
    if spec is None:
        return None, None
    parts = spec.split(",")
    if len(parts) == 3 and all(x.strip().isdigit() for x in parts):
        c = tuple(int(x) for x in parts)
        if any(x > 255 for x in c):
            raise SystemExit("eval_cli: --composite colour components are 0..255, got %s" % spec)
        return c, None
    if not os.path.exists(spec):
        raise SystemExit("eval_cli: --composite %s is neither R,G,B nor an existing image" % spec)
    return None, spec


def parse_mask_options(band, thresholds):
    """--mask-band "R[,R_BG]" -> r | (r_fg, r_bg) | None, --mask-thresholds "LO,HI" -> (lo, hi); both checked as masks.Mask does."""
    from .masks import band_thresholds, check_thresholds
    try:
        b = None
        if band is not None:
            parts = [float(x) for x in band.split(",")]
            if len(parts) not in (1, 2):
                raise ValueError("one or two radii")
            b = parts[0] if len(parts) == 1 else tuple(parts)
            band_thresholds(b)
    except ValueError as e:
        raise SystemExit("eval_cli: --mask-band is R or R,R_BG with radii in 0 ... 255 pixels, got %r (%s)" % (band, e))
    try:
        lo, hi = (int(x) for x in thresholds.split(","))
        check_thresholds(lo, hi)
    except ValueError as e:
        raise SystemExit("eval_cli: --mask-thresholds is LO,HI with 0 <= LO < HI <= 255, got %r (%s)" % (thresholds, e))
    return b, (lo, hi)


def parse_stabilise_options(strength, taus, region):
    """--stabilise [K], --stabilise-taus "C,A", --stabilise-region -> run_video_matte's ``stabilise`` dict (None when --stabilise
    was not given); checked as temporal.TemporalStabiliser does."""
    from .temporal import check_options
    if strength is None:
        if taus is not None or region is not None:
            raise SystemExit("eval_cli: --stabilise-taus / --stabilise-region belong to --stabilise")
        return None
    kw = {"strength": strength}
    if taus is not None:
        try:
            kw["tau_colour"], kw["tau_alpha"] = (float(x) for x in taus.split(","))
        except ValueError as e:
            raise SystemExit("eval_cli: --stabilise-taus is C,A (grey levels, alpha), both positive, got %r (%s)" % (taus, e))
    if region is not None:
        kw["region"] = region
    try:
        check_options(**kw)
    except ValueError as e:
        raise SystemExit("eval_cli: --stabilise K takes a strength in [0,1], --stabilise-taus C,A two positive numbers (%s)" % e)
    return kw


def parse_roi_options(roi, margin):
    """--roi "auto" | "track[,H,W]" | "Y0,X0,H,W", --roi-margin M -> run_video_matte's (roi, roi_margin); (None, 32) when --roi was not given."""
    if roi is None:
        if margin is not None:
            raise SystemExit("eval_cli: --roi-margin belongs to --roi")
        return None, 32
    if margin is not None and margin < 0:
        raise SystemExit("eval_cli: --roi-margin is a number of pixels >= 0, got %d" % margin)
    if roi == "track" or roi.startswith("track,"):
        parts = roi.split(",")[1:]
        if parts and (len(parts) != 2 or not all(x.strip().isdigit() and int(x) >= 1 for x in parts)):
            raise SystemExit("eval_cli: --roi track takes no size or one, track,H,W (pixels, H and W at least 1), got %r" % roi)
        roi = ("track",) + tuple(int(x) for x in parts) if parts else "track"
    elif roi != "auto":
        parts = roi.split(",")
        if len(parts) != 4 or not all(x.strip().isdigit() for x in parts) or int(parts[2]) < 1 or int(parts[3]) < 1:
            raise SystemExit("eval_cli: --roi is auto, track[,H,W] or a window Y0,X0,H,W (pixels, H and W at least 1), got %r" % roi)
        roi = tuple(int(x) for x in parts)
    return roi, 32 if margin is None else margin


def add_key_arguments(ap):
    """--key / --plate and their options, for every command line that takes them (parse_key_options reads them back)"""
    ap.add_argument("--key", default=None, metavar="green|blue|R,G,B",
                    help="trimap-free matting of footage shot against a screen: every frame's mask is keyed on the device from "
                         "the frame itself (a hue-cone chroma key), then made into a trimap as a mask is")
    ap.add_argument("--key-thresholds", default=None, metavar="LO,HI",
                    help="--key: subject up to LO, screen from HI, in chroma code values (default 8,24: placeholders, not tuned on "
                         "real footage)")
    ap.add_argument("--plate", default=None, metavar="PATH",
                    help="trimap-free matting of a locked-off shot: every frame's mask is its difference to this clean plate of the "
                         "empty set (an image of the frames' resolution)")
    ap.add_argument("--plate-thresholds", default=None, metavar="LO,HI",
                    help="--plate: plate up to LO, subject from HI, 0 <= LO < HI <= 255 (default 12,40: placeholders)")
    ap.add_argument("--plate-radius", type=int, default=None, metavar="R",
                    help="--plate: the plate is searched in a (2R+1)^2 neighbourhood, R in 0 ... 3 (default 1: a placeholder)")


def parse_key_options(args, who="eval_cli"):
    """--key green|blue|R,G,B [--key-thresholds LO,HI] | --plate PATH [--plate-thresholds LO,HI] [--plate-radius R] -> None, or
    make(band, mask_lo, mask_hi, H, W, rgb) -> run_video_matte's ``key`` (the plate is read, once, when the frames' size and channel
    order are known).  Everything that needs no image is checked here, as keys.ChromaKey / keys.PlateKey do."""
    from . import keys
    if args.key is not None and args.plate is not None:
        raise SystemExit("%s: --key and --plate exclude each other (one key makes the mask)" % who)
    if args.key is None and args.key_thresholds is not None:
        raise SystemExit("%s: --key-thresholds belongs to --key" % who)
    if args.plate is None and (args.plate_thresholds is not None or args.plate_radius is not None):
        raise SystemExit("%s: --plate-thresholds / --plate-radius belong to --plate" % who)
    if args.key is None and args.plate is None:
        return None
    if args.key is not None:
        colour = args.key
        if colour not in keys.COLOURS:
            parts = colour.split(",")
            if len(parts) != 3 or not all(x.strip().isdigit() and int(x) <= 255 for x in parts):
                raise SystemExit("%s: --key is green, blue or R,G,B (0..255), got %r" % (who, args.key))
            colour = tuple(int(x) for x in parts)
        kw = {}
        if args.key_thresholds is not None:
            try:
                kw["lo"], kw["hi"] = (float(x) for x in args.key_thresholds.split(","))
            except ValueError:
                raise SystemExit("%s: --key-thresholds is LO,HI with LO < HI, got %r" % (who, args.key_thresholds))
        try:
            keys.ChromaKey(colour, **kw)
        except ValueError as e:
            raise SystemExit("%s: --key: %s" % (who, e))
        return lambda band, mask_lo, mask_hi, H, W, rgb: keys.ChromaKey(colour, band=band, mask_lo=mask_lo, mask_hi=mask_hi, **kw)
    kw = {}
    if args.plate_thresholds is not None:
        try:
            kw["lo"], kw["hi"] = (int(x) for x in args.plate_thresholds.split(","))
            if not 0 <= kw["lo"] < kw["hi"] <= 255:
                raise ValueError
        except ValueError:
            raise SystemExit("%s: --plate-thresholds is LO,HI with 0 <= LO < HI <= 255, got %r" % (who, args.plate_thresholds))
    if args.plate_radius is not None:
        if not 0 <= args.plate_radius <= 3:
            raise SystemExit("%s: --plate-radius is 0 ... 3, got %d" % (who, args.plate_radius))
        kw["radius"] = args.plate_radius
    if not os.path.exists(args.plate):
        raise SystemExit("%s: --plate %s is not an existing image" % (who, args.plate))
    path = args.plate

    def make(band, mask_lo, mask_hi, H, W, rgb):
        import numpy as np
        from PIL import Image
        arr = np.asarray(Image.open(path).convert("RGB"))
        if arr.shape[:2] != (H, W):
            raise SystemExit("%s: --plate %s is %dx%d, the frames are %dx%d (a plate is given at the frames' resolution)"
                             % (who, path, arr.shape[1], arr.shape[0], W, H))
        return keys.PlateKey(np.ascontiguousarray(arr if rgb else arr[..., ::-1]), band=band, mask_lo=mask_lo, mask_hi=mask_hi, **kw)
    return make


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True)
    ap.add_argument("--out", default="./demo_results")
    ap.add_argument("--demo", action="store_true", help="demo layout; default: VideoMatting108 validation split")
    ap.add_argument("--subset", action="store_true", help="VideoMatting108: val_videos_subset.txt")
    ap.add_argument("--viz", action="store_true", help="also write the six-panel composites (eval.py --viz)")
    ap.add_argument("--fgr", action="store_true", help="also write the foreground estimate as RGBA PNGs (<out>/fgr/<seq>/)")
    ap.add_argument("--composite", default=None, metavar="PATH|R,G,B",
                    help="also write the foreground composited over a new background image or colour (<out>/comp/<seq>/)")
    ap.add_argument("--keyframes", action="store_true",
                    help="demo layout: use every trimap/<stem>.png as a full keyframe and every labels/<stem>.png as a correction")
    ap.add_argument("--work-scale", type=int, default=None, choices=[2, 3, 4],
                    help="demo layout: run the network on an S x S block mean of the frames, guided upsampling back to their resolution")
    ap.add_argument("--work-radius", type=int, default=2, help="--work-scale: guided-filter radius in working pixels, 1 ... 4")
    ap.add_argument("--work-eps", type=float, default=1e-4, help="--work-scale: guided-filter regulariser on the [0,1] scale")
    ap.add_argument("--masks", default=None, choices=["key", "frame"],
                    help="demo layout: trimaps from the segmentation masks mask/<stem>.png; key = every mask is a full keyframe, "
                         "frame = every frame is matted from its own mask, nothing propagated")
    ap.add_argument("--mask-band", default=None, metavar="R[,R_BG]",
                    help="--masks: reach of the unknown band into foreground / background in pixels (default: the --trimap dilation)")
    ap.add_argument("--mask-thresholds", default="127,128", metavar="LO,HI",
                    help="--masks: foreground is mask >= HI, background mask <= LO (8-bit scale)")
    add_key_arguments(ap)
    ap.add_argument("--stabilise", type=float, nargs="?", const=0.5, default=None, metavar="K",
                    help="demo layout: temporal stabilisation of alpha, a flow-compensated recursive filter of strength K in [0,1] "
                         "(default 0.5: a placeholder, not tuned on real footage)")
    ap.add_argument("--stabilise-taus", default=None, metavar="C,A",
                    help="--stabilise: the grey residual (8-bit levels) and the change of alpha at which the filter lets go "
                         "(default 24,0.5: placeholders)")
    ap.add_argument("--stabilise-region", default=None, choices=["unknown", "all"],
                    help="--stabilise: filter only the trimap's unknown class (default) or every pixel")
    ap.add_argument("--roi", default=None, metavar="auto|track[,H,W]|Y0,X0,H,W",
                    help="demo layout: run the network in a window round the subject and paste the result back (the matte of the "
                         "cropped clip, not the full-frame matte); auto places the window from the trimaps / masks, track lets it "
                         "follow the propagated trimap, one frame behind")
    ap.add_argument("--roi-margin", type=int, default=None, metavar="M",
                    help="--roi auto: pixels kept round the subject's box (default 32: a placeholder, not tuned on real footage)")
    ap.add_argument("--subjects", action="store_true",
                    help="demo layout: one matte per subject -- every sub-directory of <seq>/subjects/ holds one subject's first-frame "
                         "trimap; the subjects' tracking windows run as one lock-step batch (--roi track[,H,W], or no --roi: "
                         "full frames)")
    ap.add_argument("--subjects-overlap", default=None, choices=["keep", "normalise"],
                    help="--subjects: where windows overlap keep every subject's alpha (default) or divide the alphas of a pixel by "
                         "their sum where it exceeds 1 (a placeholder rule, not tuned on real footage)")
    ap.add_argument("--max-frames", type=int, default=None, help="only the first N frames of every sequence")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--trimap", default="medium", choices=["narrow", "medium", "wide"])
    ap.add_argument("--skip", type=int, default=10)          # cfg.TEST.MEMORY_SKIP_FRAME (config.py:23)
    ap.add_argument("--max-num", type=int, default=5)        # cfg.TEST.MEMORY_MAX_NUM   (config.py:22)
    ap.add_argument("--precision", default=None, choices=["f32", "f16x3", "f16"],
                    help="f16x3 (default, fp32-class), f32 (exact-fp32 MFMA), f16 (one fp16 MFMA pass: reduced precision, labelled mode)")
    ap.add_argument("--gpus", type=int, default=None, help="start this many ranks, one per GPU (default: the launcher's)")
    ap.add_argument("--sync-io", action="store_true", help="write PNGs synchronously in the frame loop (as eval.py does)")
    ap.add_argument("--batch", type=int, default=None,
                    help="sequences of equal resolution stepped in lock-step per GPU (one launch per layer over the batch; "
                         "frames are decoded up front in this mode).  Default: 1 for a single rank; a multi-rank run "
                         "(--gpus N / torchrun: a throughput run, configs[3]) picks 2 at 1080p and 4 at <= 480p "
                         "(dist.default_batch; measured +5 % / +41 % aggregate)")
    ap.add_argument("--all-metrics", action="store_true",
                    help="VideoMatting108: also Grad, Conn and SSDA against the ground truth (device kernels, metric.py:191-250)")
    ap.add_argument("--messddt", action="store_true",
                    help="VideoMatting108: also MESSDdt against the ground truth (Farneback flow on the device, metric.py:266-302)")
    ap.add_argument("--summary-json", default=None, help="rank 0 writes the reduced summary (frames, fps, metrics, shards) here")
    args = ap.parse_args(argv)
    from PIL import Image
    from . import helpers
    from .dist import run_sharded, self_launch_command
    from .io_pipeline import AlphaWriter, FramePrefetcher, _Listish
    from .video import run_video_matte

    comp_color, comp_image = parse_composite(args.composite)
    mask_band, (mask_lo, mask_hi) = parse_mask_options(args.mask_band, args.mask_thresholds)
    stabilise = parse_stabilise_options(args.stabilise, args.stabilise_taus, args.stabilise_region)
    if stabilise is not None and not args.demo:
        raise SystemExit("eval_cli: --stabilise belongs to the demo routes (the VideoMatting108 flow composites every frame over a "
                         "background of its own); add --demo")
    if stabilise is not None and args.batch is not None and args.batch > 1:
        raise SystemExit("eval_cli: --batch %d steps clips in lock-step through matte_batch, which does not implement --stabilise"
                         % args.batch)
    if stabilise is not None and args.viz:
        raise SystemExit("eval_cli: --stabilise changes alpha behind the frame; the --viz panels show the network's own outputs: "
                         "drop one of them")
    roi, roi_margin = parse_roi_options(args.roi, args.roi_margin)
    if roi is not None and not args.demo:
        raise SystemExit("eval_cli: --roi belongs to the demo routes (the window is placed round a trimap's classes; the "
                         "VideoMatting108 flow derives its trimap from the ground truth); add --demo")
    if roi is not None and args.batch is not None and args.batch > 1:
        raise SystemExit("eval_cli: --batch %d steps clips in lock-step through matte_batch, which does not implement --roi"
                         % args.batch)
    if roi is not None and args.viz:
        raise SystemExit("eval_cli: --roi pastes alpha into the frame behind the network; the --viz panels show the network's own "
                         "outputs, at the window's size: drop one of them")
    if roi is not None and args.work_scale is not None:
        raise SystemExit("eval_cli: --roi and --work-scale exclude each other (a window at the working resolution is out of scope)")
    if args.masks and not args.demo:
        raise SystemExit("eval_cli: --masks reads the demo layout's mask/ folder; add --demo")
    if args.masks == "frame" and roi is not None and (roi == "track" or roi[0] == "track"):
        raise SystemExit("eval_cli: --roi track follows a propagated trimap; --masks frame propagates nothing, and --roi auto already "
                         "tracks there")
    if args.masks and args.batch is not None and args.batch > 1:
        raise SystemExit("eval_cli: --batch %d steps clips in lock-step through matte_batch, which does not implement --masks"
                         % args.batch)
    if args.masks == "frame" and args.keyframes:
        raise SystemExit("eval_cli: --masks frame mattes every frame from its own mask and propagates nothing: there is no trimap "
                         "for --keyframes to place or correct; use --masks key")

    make_key = parse_key_options(args)
    if make_key is not None:
        flag = "--key" if args.key is not None else "--plate"
        if not args.demo:
            raise SystemExit("eval_cli: %s belongs to the demo routes (the VideoMatting108 flow derives its trimap from the ground "
                             "truth); add --demo" % flag)
        for on, other in ((args.masks, "--masks"), (args.keyframes, "--keyframes"), (args.subjects, "--subjects"),
                          (args.batch is not None and args.batch > 1, "--batch > 1")):
            if on:
                raise SystemExit("eval_cli: %s mattes every frame of ONE clip from the trimap of its own key and excludes %s"
                                 % (flag, other))
        if roi is not None and (roi == "track" or roi[0] == "track"):
            raise SystemExit("eval_cli: --roi track follows a propagated trimap; %s propagates nothing, and --roi auto already "
                             "tracks there" % flag)

    if args.subjects_overlap is not None and not args.subjects:
        raise SystemExit("eval_cli: --subjects-overlap belongs to --subjects")
    if args.subjects:
        if not args.demo:
            raise SystemExit("eval_cli: --subjects reads the demo layout's subjects/ folder (a first-frame trimap per subject); add --demo")
        if roi is not None and not (roi == "track" or roi[0] == "track"):
            raise SystemExit("eval_cli: --subjects follows every subject with a tracking window of its own, all of one size: --roi "
                             "track[,H,W] or no --roi (full frames); --roi auto and a static window belong to single-subject clips")
        for on, flag in ((args.keyframes, "--keyframes"), (args.masks, "--masks"), (args.work_scale is not None, "--work-scale"),
                         (stabilise is not None, "--stabilise"), (args.viz, "--viz"), (args.composite is not None, "--composite"),
                         (args.batch is not None and args.batch > 1, "--batch > 1")):
            if on:
                raise SystemExit("eval_cli: --subjects mattes the subjects of ONE clip in lock-step through run_video_matte_subjects, "
                                 "which does not implement %s" % flag)

    if args.gpus is not None and args.gpus > 1 and "RANK" not in os.environ:
        import subprocess
        import sys
        cmd = self_launch_command(args.gpus, os.environ, torch.cuda.device_count(), "-m",
                                  ["otvm_amd.eval_cli"] + list(sys.argv[1:] if argv is None else argv))
        raise SystemExit(subprocess.call(cmd))

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("OTVM_DIST_BACKEND", "nccl") != "nccl":
        local_rank %= max(1, torch.cuda.device_count())     # gloo rehearsal: more ranks than GPUs share the devices round-robin
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    # under a launcher (also with ONE rank: RCCL initialised and used).  A stray RANK variable alone is not a launcher: without
    # the rendezvous variables init_process_group would hang or fail where a plain process ran before
    distributed = world > 1 or all(k in os.environ for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"))
    if distributed:
        # one process per GPU, RCCL for the final metric reduction; OTVM_DIST_BACKEND=gloo rehearses the multi-rank path with
        # several ranks on ONE GPU (RCCL refuses that).  Each rank -- its launch thread and the IO pools it starts -- gets
        # its own share of the node's cores.
        from .dist import init_process_group, pin_rank_affinity
        init_process_group(dev)
        pin_rank_affinity(int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    dk = {"narrow": 5, "medium": 12, "wide": 20}[args.trimap]              # eval.py:67-72
    cfg = helpers.default_cfg()
    model = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", dk), "Test", dk)
    if args.synthetic_weights:
        from .synth_weights import synthetic_state_dict
        model.load_state_dict(synthetic_state_dict(0), strict=True)
    else:
        model.load_state_dict(torch.load(args.weights, map_location="cpu"), strict=True)     # eval.py:77-79
    model.precision = args.precision
    # eval.py:80 wraps the model in nn.DataParallel with ONE visible device (CUDA_VISIBLE_DEVICES, eval.py:42).  Under a
    # launcher every GPU is visible to every rank, so the wrapper is pinned to this rank's device: with the default
    # device_ids it would scatter the frames over all GPUs and its per-call replicas would lose the memory bank.
    model = torch.nn.DataParallel(model.to(dev), device_ids=[dev.index], output_device=dev.index).eval()
    from . import datasets, viz
    ds = datasets.Demo_Test(args.data) if args.demo else datasets.VideoMatting108_Test(args.data, mode="val",
                                                                                       use_subset=args.subset)
    items = list(ds)
    seqs = [dict(name=it[6], frames=it[2][:args.max_frames], item=it) for it in items]   # paths: sharding by length
    root_out = os.path.join(args.out, "alpha", "test", helpers.get_model_name(cfg))

    def resolution(sq):
        if not sq["frames"]:
            return None                                   # an empty sequence has no resolution (and is never batched with another)
        with Image.open(os.path.join(sq["item"][1], sq["frames"][0])) as im:
            return (im.height, im.width)
    keys = [resolution(sq) for sq in seqs]
    if args.batch is None:
        # a multi-rank run is a throughput run: lock-step batches by default, sized by the largest resolution in the set
        from .dist import default_batch
        from .engine import pad_amounts
        args.batch = 1
        # (--viz and --sync-io are single-clip features -- matte_batch writes no viz frames and decodes every clip of a group up
        #  front -- so they keep batch 1 unless --batch is given explicitly)
        if world > 1 and any(k is not None for k in keys) and not (args.viz or args.sync_io or args.fgr or args.composite
                                                                   or args.keyframes or args.masks or stabilise is not None
                                                                   or roi is not None or args.subjects or make_key is not None):
            def padded(k):
                lw, uw, lh, uh = pad_amounts(k[0], k[1], 32)
                return (k[0] + lh + uh) * (k[1] + lw + uw)
            args.batch = default_batch(max(padded(k) for k in keys if k is not None))
    if args.batch > 1 and (args.viz or args.sync_io):
        raise SystemExit("eval_cli: --batch %d steps clips in lock-step through matte_batch, which implements neither --viz nor "
                         "--sync-io; drop one of them" % args.batch)
    if args.batch > 1 and (args.fgr or args.composite):
        raise SystemExit("eval_cli: --batch %d steps clips in lock-step through matte_batch, which implements neither --fgr nor "
                         "--composite; drop one of them" % args.batch)
    if args.keyframes and not args.demo:
        raise SystemExit("eval_cli: --keyframes reads the demo layout's trimap/ and labels/ folders; add --demo")
    if args.keyframes and args.batch > 1:
        raise SystemExit("eval_cli: --batch %d steps clips in lock-step through matte_batch, which does not implement --keyframes"
                         % args.batch)
    if args.work_scale is not None and not args.demo:
        raise SystemExit("eval_cli: --work-scale belongs to the trimap (demo) flow; add --demo")
    if args.work_scale is not None and (args.batch > 1 or args.viz):
        raise SystemExit("eval_cli: --work-scale is a single-clip route without the --viz panels; drop --batch %d / --viz" % args.batch)
    if rank == 0:
        print("eval_cli: %d rank(s), lock-step batch %d per rank" % (world, args.batch))
    if distributed:
        # every rank must launch the same kernel configurations, or a clip's alpha (fp32 summation order) would depend on
        # the rank that got it: rank 0 builds -- and times -- the plans of all resolutions in the data set, the others adopt
        # its choices (engine.share_tune_cache) before they build theirs
        # (the tuner's signature carries the batch size: every (resolution, group size) any rank will step is built here)
        from .dist import planned_batch_shapes
        from .engine import share_tune_cache
        if rank == 0:
            eng = model.module._get_engine()
            shapes = planned_batch_shapes([len(sq["frames"]) for sq in seqs], keys, world, max(1, args.batch))
            for (k, b_) in sorted(s_ for s_ in shapes if s_[0] is not None):
                eng.plan(k[0], k[1], b_)
            torch.cuda.synchronize(dev)
        share_tune_cache(0)

    roi_state = {"size": None}                        # --roi: the window size of the previous clip

    def matte_subjects(seq):
        """--subjects: every sub-directory of <seq>/subjects/ is one subject, in sorted order; its trimap is the PNG carrying the
        first frame's stem, decoded as trimap/ is.  Per-subject alphas under <pred>/<seq>/<subject>/, the union at <pred>/<seq>/
        (the usual place), with --fgr the RGBA under <out>/fgr/<seq>/<subject>/."""
        from .subjects import run_video_matte_subjects
        from .video import trimap_file_to_onehot
        data = datasets.load_sequence(seq["item"], max_frames=args.max_frames, decode_frames=True, masks=True)   # (no trimap/ needed)
        names, sdir = data["names"], os.path.join(seq["item"][1], seq["name"], "subjects")
        who = sorted(d for d in os.listdir(sdir) if os.path.isdir(os.path.join(sdir, d))) if os.path.isdir(sdir) else []
        if not who or not names:
            raise SystemExit("eval_cli: --subjects found no subject for sequence %s (%s/<subject>/<first frame>.png)" % (seq["name"], sdir))
        missing = [n for n in who if not os.path.isfile(os.path.join(sdir, n, names[0] + ".png"))]
        if missing:
            raise SystemExit("eval_cli: sequence %s: no first-frame trimap %s.png for subject(s) %s" % (seq["name"], names[0], ", ".join(missing)))
        tris = [trimap_file_to_onehot(datasets.read_trimap_unchanged(os.path.join(sdir, n, names[0] + ".png"))) for n in who]
        try:
            res = run_video_matte_subjects(model, data["frames"], tris, roi=roi, roi_margin=roi_margin,
                                           overlap=args.subjects_overlap or "keep", skip=args.skip, max_num=args.max_num,
                                           frames_are_rgb=False, foreground=args.fgr, device=dev)
        except ValueError as e:
            raise SystemExit("eval_cli: sequence %s: %s" % (seq["name"], e))
        outdir = os.path.join(root_out, "pred", seq["name"])
        for s, n in enumerate([None] + who):
            planes = res["union_u8"] if n is None else res["alpha_u8"][s - 1]
            d = outdir if n is None else os.path.join(outdir, n)
            os.makedirs(d, exist_ok=True)
            for t, stem in enumerate(names):
                Image.fromarray(planes[t].numpy()).save(os.path.join(d, stem + ".png"))
                if args.fgr and n is not None:
                    fd = os.path.join(args.out, "fgr", seq["name"], n)
                    os.makedirs(fd, exist_ok=True)
                    rgba = res["fgr_u8"][s - 1, t].numpy()                      # the frames are decoded B, G, R here
                    Image.fromarray(rgba[..., [2, 1, 0, 3]].copy()).save(os.path.join(fd, stem + ".png"))
        # every (window size, S) is a frame plan of its own and nothing else evicts them (as --roi)
        key = [list(res["roi_size"]), len(who)]
        if roi_state["size"] is not None and roi_state["size"] != key:
            model.module.drop_plans()
        roi_state["size"] = key
        return dict(subjects=who, roi=[[list(w) for w in ws] for ws in res["roi"]], roi_size=list(res["roi_size"]),
                    roi_clipped=res["roi_clipped"], bank_frames=res["bank_frames"])

    def matte(seq):
        if args.subjects:
            return matte_subjects(seq)
        demo = seq["item"][0] == "demo"
        keyed = demo and (args.keyframes or args.masks == "key")   # frames in schedule order: decoded up front, not prefetched
        data = datasets.load_sequence(seq["item"], max_frames=args.max_frames, decode_frames=not demo or args.sync_io or keyed,
                                      keyframes=demo and args.keyframes,
                                      masks=demo and (bool(args.masks) or make_key is not None))   # (a key needs no trimap/)
        outdir = os.path.join(root_out, "pred", seq["name"])
        os.makedirs(outdir, exist_ok=True)
        vizdir = os.path.join(args.out, "viz", "test", helpers.get_model_name(cfg), "viz", seq["name"])
        if args.viz:
            os.makedirs(vizdir, exist_ok=True)
        writer = None if args.sync_io else AlphaWriter(dev, outdir, [n + ".png" for n in data["names"]])
        # foreground outputs: writers of their own (asynchronous also with --sync-io: only the alpha path mirrors eval.py's loop)
        png_names = [n + ".png" for n in data["names"]]
        want_fgr = args.fgr or args.composite is not None
        fwriter = AlphaWriter(dev, os.path.join(args.out, "fgr", seq["name"]), png_names) if args.fgr else None
        cwriter = AlphaWriter(dev, os.path.join(args.out, "comp", seq["name"]), png_names) if args.composite is not None else None
        eng_of = model.module
        # --work-scale and --stabilise remake the foreground bytes behind the engine: they arrive through on_foreground
        # (--roi: the engine's are at the window's size; the full-resolution ones likewise)
        late_bytes = args.work_scale is not None or stabilise is not None or roi is not None
        bgr = not (demo and not args.sync_io and not keyed)   # the prefetcher hands out RGB frames, the decoded arrays are BGR

        def new_background():
            if args.composite is None:
                return None
            if comp_image is None:
                return comp_color[::-1] if bgr else comp_color
            hw = resolution(seq)
            if hw is None:
                return None                                # an empty sequence: nothing to composite
            import numpy as np
            arr = np.asarray(Image.open(comp_image).convert("RGB").resize((hw[1], hw[0]), Image.BILINEAR))   # once per clip, on the host
            return np.ascontiguousarray(arr[..., ::-1] if bgr else arr)

        def save(i, alpha, u8, out):
            if writer is None:
                Image.fromarray(u8.cpu().numpy()).save(os.path.join(outdir, data["names"][i] + ".png"))
            else:
                writer.put(i, u8)
            if fwriter is not None and not late_bytes:
                fwriter.put(i, eng_of._engine.last_rgba_u8, bgr=bgr)
            if cwriter is not None and not late_bytes:
                cwriter.put(i, eng_of._engine.last_comp_u8, bgr=bgr)
            if args.viz:
                viz.write_viz_frame(os.path.join(vizdir, "f%d.jpg" % i), out)
        def save_full(i, rgba, comp):
            # --work-scale: the engine's foreground bytes are at the working resolution; the full-resolution ones arrive here,
            # frame by frame, and go to the writers as the others do (--stabilise: those of the stabilised alpha)
            if fwriter is not None:
                fwriter.put(i, rgba, bgr=bgr)
            if cwriter is not None:
                cwriter.put(i, comp, bgr=bgr)
        if demo:
            if args.sync_io or keyed:
                frames, rgb, pre = data["frames"], False, None
            else:                                  # decode ahead + pinned upload on a copy stream (RGB order)
                pre = FramePrefetcher(data["frame_paths"], dev)
                frames, rgb = _Listish(pre), True
            kf = {**data["keyframe_trimaps"], **data["label_maps"]} if args.keyframes else ({} if keyed else None)
            both = args.keyframes and sorted(set(data["keyframe_trimaps"]) & set(data["label_maps"]))
            if both:
                raise SystemExit("eval_cli: sequence %s has a trimap AND a label map for frame(s) %s" % (seq["name"], both))
            per_frame = None
            if args.masks:
                from .masks import Mask
                mk = {t: Mask(m, band=mask_band, lo=mask_lo, hi=mask_hi) for t, m in data["mask_maps"].items()}
                if args.masks == "frame":
                    missing = [n for t, n in enumerate(data["names"]) if t not in mk]
                    if missing:
                        raise SystemExit("eval_cli: --masks frame needs a mask for every frame; sequence %s has none for %s"
                                         % (seq["name"], ", ".join(missing[:5]) + (" ..." if len(missing) > 5 else "")))
                    per_frame = [mk[t] for t in range(len(data["names"]))]
                else:
                    if not args.keyframes and data["trimap"] is not None:
                        kf[0] = data["trimap"]               # (without --keyframes only the first frame's trimap file counts)
                    both = sorted(set(kf) & set(mk))
                    if both:
                        raise SystemExit("eval_cli: sequence %s has a mask AND a trimap or label map for frame(s) %s"
                                         % (seq["name"], both))
                    kf.update(mk)
                    if not (mk or (data["keyframe_trimaps"] if args.keyframes else data["trimap"] is not None)):
                        raise SystemExit("eval_cli: sequence %s has neither a trimap nor a mask on any frame (%s/%s/trimap|mask/"
                                         "<frame>.png)" % (seq["name"], seq["item"][1], seq["name"]))
            clip_key = None
            if make_key is not None and resolution(seq) is not None:
                # --roi auto reads every frame twice: the decoded list can be, the prefetcher cannot
                if roi == "auto" and pre is not None:
                    pre.close()
                    data = datasets.load_sequence(seq["item"], max_frames=args.max_frames, decode_frames=True, masks=True)
                    frames, rgb, pre, bgr = data["frames"], False, None, True
                clip_key = make_key(mask_band, mask_lo, mask_hi, *resolution(seq), rgb)
            res = run_video_matte(model, frames, trimap=None if (keyed or per_frame is not None or clip_key is not None) else data["trimap"],
                                  skip=args.skip, max_num=args.max_num, masks=per_frame, key=clip_key,
                                  on_frame=save, device=dev, frames_are_rgb=rgb, keep_on_device=True,
                                  foreground=want_fgr, new_background=new_background(), keyframes=kf,
                                  stabilise=stabilise, **(dict(roi=roi, roi_margin=roi_margin) if roi is not None else {}),
                                  **(dict(on_foreground=save_full if want_fgr else None) if late_bytes else {}),
                                  **(dict(work_scale=args.work_scale, work_radius=args.work_radius, work_eps=args.work_eps)
                                     if args.work_scale is not None else {}))
            if pre is not None:
                pre.close()
            if args.work_scale is not None:
                res["work_scale"], res["work_size"] = args.work_scale, list(res["work_size"] or ())
            if roi is not None:
                res["roi"] = [list(w) for w in res["roi"]]
                res["roi_size"] = list(res["roi_size"] or ())
                # every window size is a frame plan of its own and nothing else evicts them: when this clip's size differs from
                # the previous clip's, the engine's plans are dropped before the next clip (it plans again at its own size)
                if roi_state["size"] is not None and res["roi_size"] and roi_state["size"] != res["roi_size"]:
                    model.module.drop_plans()
                roi_state["size"] = res["roi_size"] or roi_state["size"]
        else:
            res = run_video_matte(model, data["frames"], alphas=data["alphas"], backgrounds=data["backgrounds"],
                                  skip=args.skip, max_num=args.max_num, on_frame=save, device=dev,
                                  gt_alpha_u8=data["gt_alpha_u8"], gt_mask="unknown", keep_on_device=True,
                                  gt_image_metrics=args.all_metrics, gt_flow_metrics=args.messddt,
                                  foreground=want_fgr, new_background=new_background())
        if writer is not None:
            writer.close()
        for w in (fwriter, cwriter):
            if w is not None:
                w.close()
        for k in ("fgr_u8", "comp_u8", "alpha_raw"):
            res.pop(k, None)                       # written as PNGs; the per-clip results keep today's keys
        if args.viz:
            viz.make_viz_video(os.path.join(vizdir, "f%d.jpg"),                          # eval.py:229-242
                               os.path.join(args.out, "viz", "test", helpers.get_model_name(cfg), "viz",
                                            seq["name"].replace("/", "_") + ".mp4"))
        return res
    def matte_batch(group):
        """--batch: the clips of ``group`` (one resolution) in lock-step; PNGs through one asynchronous writer per clip."""
        from .video import run_video_matte_batch
        datas = [datasets.load_sequence(sq["item"], max_frames=args.max_frames, decode_frames=True) for sq in group]
        writers = []
        for sq, data in zip(group, datas):
            outdir = os.path.join(root_out, "pred", sq["name"])
            os.makedirs(outdir, exist_ok=True)
            writers.append(AlphaWriter(dev, outdir, [n + ".png" for n in data["names"]]))
        save = lambda b, i, alpha, u8, out: writers[b].put(i, u8)
        if group[0]["item"][0] == "demo":
            res = run_video_matte_batch(model, [d["frames"] for d in datas], trimaps=[d["trimap"] for d in datas], skip=args.skip,
                                        max_num=args.max_num, on_frame=save, device=dev, keep_on_device=True)
        else:
            res = run_video_matte_batch(model, [d["frames"] for d in datas], alphas=[d["alphas"] for d in datas],
                                        backgrounds=[d["backgrounds"] for d in datas], skip=args.skip, max_num=args.max_num,
                                        on_frame=save, device=dev, keep_on_device=True,
                                        gt_alpha_u8=[d["gt_alpha_u8"] for d in datas], gt_mask="unknown",
                                        gt_image_metrics=args.all_metrics, gt_flow_metrics=args.messddt)
        for w in writers:
            w.close()
        return res

    from .dist import reduce_device
    summary = run_sharded(seqs, matte, rank=rank, world=world, device=reduce_device(dev) if distributed else dev,
                          batch=max(1, args.batch), matte_batch_fn=matte_batch, key_fn=resolution)
    if args.work_scale is not None:
        # (the working sizes of the sequences this rank matted; a single-rank run lists them all)
        summary["work_scale"] = args.work_scale
        summary["work_size"] = {seqs[i]["name"]: o["work_size"] for i, o in summary["outputs"].items() if o.get("work_size")}
    if args.masks:
        summary["masks"] = args.masks
        summary["mask_band"] = list(mask_band) if isinstance(mask_band, tuple) else [dk if mask_band is None else mask_band] * 2
        summary["mask_thresholds"] = [mask_lo, mask_hi]
    if make_key is not None:
        summary["key"] = args.key if args.key is not None else "plate"
    if roi is not None:
        summary["roi"], summary["roi_margin"] = (roi if isinstance(roi, str) else list(roi)), roi_margin
        summary["roi_size"] = {seqs[i]["name"]: o["roi_size"] for i, o in summary["outputs"].items() if o.get("roi_size")}
        summary["roi_clipped"] = {seqs[i]["name"]: o["roi_clipped"] for i, o in summary["outputs"].items() if "roi_clipped" in o}
    if args.subjects:
        summary["subjects"] = {seqs[i]["name"]: o["subjects"] for i, o in summary["outputs"].items() if "subjects" in o}
        summary["subjects_overlap"] = args.subjects_overlap or "keep"
    if stabilise is not None:
        summary["stabilise"] = {k: stabilise.get(k, d) for k, d in (("strength", 0.5), ("tau_colour", 24.0), ("tau_alpha", 0.5),
                                                                      ("region", "unknown"))}
    if distributed:
        import torch.distributed as dist
        # which kernel configurations this rank launched (fp32 summation orders): identical on all ranks by construction
        # (share_tune_cache), reported so that a run can prove it
        from .engine import kernel_config_digest
        digests = [None] * world
        dist.all_gather_object(digests, kernel_config_digest())
        if len(set(digests)) != 1 and rank == 0:
            import warnings
            warnings.warn("eval_cli: the ranks launched different kernel configurations (tuned choices or OTVM_* switches differ "
                          "between ranks): a clip's last bits depend on the rank that got it.  Digests: %s" % digests)
        summary["tune_digests"] = digests
        summary["batch"] = args.batch
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and args.summary_json:
        import json
        json.dump({k: v for k, v in summary.items() if k != "outputs"}, open(args.summary_json, "w"), indent=0)
    if rank == 0:
        print("done | %d frames | %.2f frames/s over %d GPU(s)" % (summary["frames"], summary["fps"], world))
        if "gt_metrics" in summary:
            g = summary["gt_metrics"]
            extra = ""
            if "grad_mean" in g:
                extra = " | Grad/frame %.4f | Conn/frame %.4f | SSDA/frame %.6f" % (g["grad_mean"], g["conn_mean"], g["ssda_mean"])
            if "messddt_mean" in g:
                extra += " | MESSDdt/pair %.6f" % g["messddt_mean"]
            print("vs ground truth (unknown band) | SAD/frame %.4f | MSE/frame %.6f (pooled %.6f) | dtSSD/pair %.6f%s | frames %d"
                  % (g["sad"], g["mse_mean"], g["mse"], g["dtssd_mean"], extra, g["frames"]))
    return summary


if __name__ == "__main__":
    main()
