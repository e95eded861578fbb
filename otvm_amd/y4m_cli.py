"""Matte a video stream: Y4M (YUV4MPEG2) in, Y4M out.

    python -m otvm_amd.y4m_cli IN.y4m|- (--trimap T.png | --mask M.png | --key green|blue|R,G,B | --plate P.png) --alpha OUT.y4m|-
            [--comp OUT2.y4m --composite R,G,B|PATH] [--frames N] [--matrix auto|601|709] [--range limited|full]
            [--key-thresholds LO,HI] [--plate-thresholds LO,HI] [--plate-radius R] [--mask-band R[,R_BG]]
            [--work-scale S] [--roi track[,H,W] | Y0,X0,H,W] [--stabilise [K]] [--skip N --max-num N]
            [--weights P | --synthetic-weights] [--precision f32|f16x3|f16]

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m otvm_amd.y4m_cli - --frames N --trimap first.png --alpha alpha.y4m
    ffmpeg -i greenscreen.mov -f yuv4mpegpipe - | python -m otvm_amd.y4m_cli - --frames N --key green --alpha a.y4m

One clip in, one or two streams out (otvm_amd/yuv.py).  The input is uploaded as it lies in the stream and converted to RGB on the
device (otvm_yuv_to_rgb); --trimap is the first frame's trimap (decoded as eval_cli decodes trimap/ files), --mask a segmentation
mask of the first frame (8-bit grey; the trimap is made on the device, otvm_amd/masks.py).  --key / --plate need no art of any
kind: every frame's mask is keyed on the device from the frame itself -- a chroma key round the screen's colour, or the difference
to a clean plate (an image of the stream's size) -- and the frame is matted from it alone (run_video_matte(key=...),
otvm_amd/keys.py; every default a PLACEHOLDER, checked by definition only); each frame is needed once, so a pipe works, and --roi is
then a window Y0,X0,H,W only (auto would read the stream twice).  --alpha receives the 8-bit alphas as a
``Cmono`` full-range stream; --comp the foreground composited over --composite (a colour, or an image resized once on the host) as
``C420jpeg`` (otvm_rgb_to_yuv420), in the input's range unless --range says otherwise.  A pipe does not say how long it is:
``-`` needs --frames N; on a file --frames takes the first N.  The header of a Y4M stream does not carry its matrix: --matrix auto
takes BT.709 at H >= 720 and BT.601 below, a CONVENTION, not a measurement.  The remaining options go to run_video_matte as its
keywords (--work-scale, --roi, --stabilise: see eval_cli).  Refused streams: ``C420paldv``, high bit depth, alpha, interlaced.
Prints one JSON line (to stderr when a stream goes to stdout): frames, frames/s including IO, sizes.
"""
import argparse
import json
import sys
import time

import torch


def main(argv=None):
    ap = argparse.ArgumentParser(prog="y4m_cli")
    ap.add_argument("input", help="a Y4M file, or - for stdin (then --frames N is required)")
    ap.add_argument("--trimap", default=None, help="the first frame's trimap, a PNG as eval_cli reads from trimap/")
    ap.add_argument("--mask", default=None, help="a segmentation mask of the first frame, 8-bit grey")
    from .eval_cli import add_key_arguments
    add_key_arguments(ap)
    ap.add_argument("--mask-band", default=None, metavar="R[,R_BG]", help="--mask / --key / --plate: the reach of the unknown band in pixels")
    ap.add_argument("--alpha", required=True, help="the alpha stream (Cmono, full range), a path or - for stdout")
    ap.add_argument("--comp", default=None, help="the composite stream (C420jpeg); needs --composite")
    ap.add_argument("--composite", default=None, metavar="R,G,B|PATH", help="the new background of --comp: a colour or an image")
    ap.add_argument("--frames", type=int, default=None, help="number of frames to read (required for a pipe)")
    ap.add_argument("--matrix", default="auto", choices=["auto", "601", "709"])
    ap.add_argument("--range", default=None, choices=["limited", "full"], help="default: the header's XCOLORRANGE, limited without one")
    ap.add_argument("--work-scale", type=int, default=None, choices=[2, 3, 4])
    ap.add_argument("--roi", default=None, metavar="track[,H,W]|Y0,X0,H,W")
    ap.add_argument("--stabilise", type=float, nargs="?", const=0.5, default=None, metavar="K")
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-num", type=int, default=5)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--precision", default=None, choices=["f32", "f16x3", "f16"])
    ap.add_argument("--trimap-dilation", default="medium", choices=["narrow", "medium", "wide"], help="the model's dilation kernel (eval_cli --trimap)")
    args = ap.parse_args(argv)

    from .eval_cli import parse_key_options, parse_mask_options
    make_key = parse_key_options(args, "y4m_cli")
    if sum(x is not None for x in (args.trimap, args.mask, make_key)) != 1:
        raise SystemExit("y4m_cli: exactly one of --trimap, --mask, --key and --plate is given")
    if args.mask_band is not None and args.trimap is not None:
        raise SystemExit("y4m_cli: --mask-band belongs to --mask, --key and --plate")
    mask_band = parse_mask_options(args.mask_band, "127,128")[0]
    if (args.comp is None) != (args.composite is None):
        raise SystemExit("y4m_cli: --comp and --composite belong together")
    if not args.synthetic_weights and args.weights is None:
        raise SystemExit("y4m_cli: --weights P or --synthetic-weights")
    if args.input == "-" and args.frames is None:
        raise SystemExit("y4m_cli: a pipe does not say how long it is: pass --frames N")
    if "-" in (args.alpha, args.comp) and args.alpha == args.comp:
        raise SystemExit("y4m_cli: only one stream can go to stdout")
    from . import datasets, helpers, yuv
    from .eval_cli import parse_composite, parse_roi_options, parse_stabilise_options
    from .video import run_video_matte, trimap_file_to_onehot
    roi, roi_margin = parse_roi_options(args.roi, None)
    tracks = roi is not None and (roi == "track" or roi[0] == "track")
    if roi is not None and make_key is None and not tracks:
        raise SystemExit("y4m_cli: --roi is track or track,H,W")
    if roi is not None and make_key is not None and (tracks or roi == "auto"):
        raise SystemExit("y4m_cli: with --key / --plate --roi is a window Y0,X0,H,W (track follows a propagated trimap, and nothing is "
                         "propagated; auto would read the stream twice)")
    stabilise = parse_stabilise_options(args.stabilise, None, None)
    comp_color, comp_image = parse_composite(args.composite)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dk = {"narrow": 5, "medium": 12, "wide": 20}[args.trimap_dilation]
    cfg = helpers.default_cfg()
    model = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", dk), "Test", dk)
    if args.synthetic_weights:
        from .synth_weights import synthetic_state_dict
        model.load_state_dict(synthetic_state_dict(0), strict=True)
    else:
        model.load_state_dict(torch.load(args.weights, map_location="cpu"), strict=True)
    model.precision = args.precision
    model = torch.nn.DataParallel(model.to(dev), device_ids=[dev.index], output_device=dev.index).eval()

    try:
        frames = yuv.Y4MFrames(args.input, dev, matrix=args.matrix, range=args.range, frames=args.frames)
    except (yuv.Y4MError, OSError) as e:
        raise SystemExit("y4m_cli: %s: %s" % (args.input, e))
    h = frames.header
    H, W, T = h.H, h.W, len(frames)
    source = {}
    if make_key is not None:
        source["key"] = make_key(mask_band, 127, 128, H, W, True)      # the frames are R, G, B
        got = (H, W)
    elif args.trimap is not None:
        source["trimap"] = trimap_file_to_onehot(datasets.read_trimap_unchanged(args.trimap))
        got = tuple(source["trimap"].shape[-2:])
    else:
        from .masks import Mask
        source["mask"] = Mask(datasets.read_mask(args.mask), band=mask_band)
        got = tuple(source["mask"].shape)
    if got != (H, W):
        raise SystemExit("y4m_cli: the stream is %dx%d, the %s %dx%d" % (W, H, "trimap" if args.trimap else "mask", got[1], got[0]))
    new_background = None
    if comp_color is not None:
        new_background = comp_color                        # the frames are R, G, B
    elif comp_image is not None:
        import numpy as np
        from PIL import Image
        new_background = np.ascontiguousarray(np.asarray(Image.open(comp_image).convert("RGB").resize((W, H), Image.BILINEAR)))

    awriter = yuv.Y4MWriter(args.alpha, dev, W, H, rate=h.F, kind="mono")
    cwriter = None
    if args.comp is not None:
        cwriter = yuv.Y4MWriter(args.comp, dev, W, H, rate=h.F, kind="420", matrix=frames.matrix, range=args.range or frames.range)
    kw = {}
    if cwriter is not None:
        kw.update(new_background=new_background, on_foreground=lambda i, rgba, comp: cwriter.put(i, comp))
    if args.work_scale is not None:
        kw["work_scale"] = args.work_scale
    if roi is not None:
        kw.update(roi=roi, roi_margin=roi_margin)
    t0 = time.time()
    try:
        run_video_matte(model, frames, skip=args.skip, max_num=args.max_num, frames_are_rgb=True, device=dev, keep_on_device=True,
                        on_frame=lambda i, alpha, u8, out: awriter.put(i, u8), stabilise=stabilise, **source, **kw)
    except (ValueError, yuv.Y4MError) as e:
        raise SystemExit("y4m_cli: %s" % e)
    finally:
        frames.close()
    awriter.close()
    if cwriter is not None:
        cwriter.close()
    torch.cuda.synchronize(dev)
    dt = time.time() - t0
    summary = dict(frames=T, fps=T / dt if dt > 0 else 0.0, width=W, height=H, chroma="C" + h.C, matrix=frames.matrix, range=frames.range,
                   in_frame_bytes=h.frame_bytes, alpha_frame_bytes=awriter.nbytes, comp_frame_bytes=None if cwriter is None else cwriter.nbytes)
    print(json.dumps(summary), file=sys.stderr if "-" in (args.alpha, args.comp) else sys.stdout, flush=True)
    return summary


if __name__ == "__main__":
    main()
