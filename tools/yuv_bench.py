"""Time the video-stream route (otvm_amd/yuv.py, csrc/yuv.hip) and write the table of profiles/yuv_bench.md:

    OTVM_TUNE_FILE=tune.json python tools/yuv_bench.py [--iters 50] [--sizes 1080x1920,2160x3840] [--clip-frames 120] [--distinct 20]
                                                       [--reps 3] [--out profiles/yuv_bench.md]

Kernels, per size (H x W): the median of --iters calls, each between two device events, three untimed calls first --
otvm_yuv_to_rgb per layout (4:2:0 planar with centre siting, the others left), otvm_rgb_to_yuv420, and as the scale for "one
streaming pass" otvm_luma_u8 (3 B in, 1 B out a pixel) and otvm_roi_crop of the whole frame (3 B in, 3 B out).
Clip, 1920x1080, one process, one model, one set of convolution configurations (set OTVM_TUNE_FILE or OTVM_AUTOTUNE=0), the routes
alternating, --reps each, host clock around work that ends in a device synchronise and closed writers:
  png     the parent's route: io_pipeline.run_video_matte_io on the frames as PNG files, alphas written as PNG files
  y4m     yuv.Y4MFrames on the same frames as one C420mpeg2 file, alphas through yuv.Y4MWriter(kind="mono") into a file
  y4m_in  the same source, no sink (where the conversion on the copy stream would show)
  device  the frames resident on the device as uint8 RGB, no sink: the device-only rate
The clip is --distinct frames of synth_data.synthetic_clip played forward and backward up to --clip-frames (generating a hundred
1080p frames on the host takes longer than everything else here); the Y4M file holds what the restatement's forward conversion
makes of them, and the PNG and device routes get the frames that file decodes to, so all four matte the same pixels."""
import argparse
import ctypes as C
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

KERNEL_LAYOUTS = [("420p", "centre"), ("nv12", "left"), ("422p", "left"), ("444p", "left"), ("mono", "left")]


def bench_kernels(H, W, iters):
    from otvm_amd import lib as L
    from otvm_amd import yuv
    lib = L.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(H + W)
    row = dict(H=H, W=W)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    for layout, siting in KERNEL_LAYOUTS:
        n = yuv.frame_bytes(H, W, layout)
        buf = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(dev)
        row["to_rgb_%s_us" % layout] = 1e3 * median_ms(
            lambda: yuv._launch_to_rgb(buf, H, W, layout, "709", "limited", siting, 1, rgb, st), iters)
        row["to_rgb_%s_mb" % layout] = (n + H * W * 3) / 1e6
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    frame = torch.empty(yuv.frame_bytes(H, W, "420p"), dtype=torch.uint8, device=dev)
    row["to_yuv420_us"] = 1e3 * median_ms(lambda: yuv._launch_to_yuv420(img, H, W, "709", "limited", 1, frame, st), iters)
    row["to_yuv420_mb"] = (frame.numel() + H * W * 3) / 1e6
    grey = torch.empty((H, W), dtype=torch.uint8, device=dev)
    row["luma_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_luma_u8(img.data_ptr(), H, W, 1, grey.data_ptr(), st), "luma_u8"), iters)
    row["luma_mb"] = H * W * 4 / 1e6
    p = L.RoiCropParams(H=H, W=W, y0=0, x0=0, h=H, w=W, frame=img.data_ptr(), frame_out=rgb.data_ptr())
    row["crop_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_roi_crop(C.byref(p), st), "roi_crop"), iters)
    row["crop_mb"] = H * W * 6 / 1e6
    return row


def make_clip(tmp, T, distinct):
    """-> (y4m path, [png paths], [RGB host arrays], trimap): the same pixels three ways."""
    from PIL import Image
    from otvm_amd import yuv
    from otvm_amd.synth_data import synthetic_clip
    from tests import yuv_ref as R
    H, W = 1080, 1920
    frames_bgr, tri = synthetic_clip(H, W, distinct, seed=7)
    packed, decoded = [], []
    for fr in frames_bgr:
        y, u, v = R.rgb_to_yuv420(fr, "709", "limited", rgb=False)
        packed.append(R.pack_frame(y, u, v))
        decoded.append(R.yuv_to_rgb(y, u, v, "420p", "709", "limited", "left", rgb=True))
    order = [k if k < distinct else 2 * distinct - 1 - k for k in (t % (2 * distinct) for t in range(T))]      # forward, backward, ...
    path = os.path.join(tmp, "clip.y4m")
    with open(path, "wb") as f:
        f.write(yuv.format_y4m_header(W, H, "30:1", C="420mpeg2"))
        for k in order:
            f.write(b"FRAME\n" + packed[k])
    stills = []
    for k in range(distinct):
        stills.append(os.path.join(tmp, "still_%03d.png" % k))
        Image.fromarray(decoded[k]).save(stills[-1], compress_level=1)
    return path, [stills[k] for k in order], [decoded[k] for k in order], tri


def bench_clip(T, distinct, reps):
    from otvm_amd import helpers, yuv
    from otvm_amd.io_pipeline import run_video_matte_io
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    dev = torch.device("cuda", 0)
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        path, pngs, host, tri = make_clip(tmp, T, distinct)
        H, W = host[0].shape[:2]
        resident = [torch.from_numpy(f).to(dev) for f in host[:distinct]]
        dclip = [resident[t % distinct] for t in range(T)]                                # (any resident frames: the rate is what counts)

        def png(n):
            out = os.path.join(tmp, "png_out")
            return run_video_matte_io(m, pngs[:n], tri, outdir=out, device=dev)

        def y4m(n, sink=True):
            src = yuv.Y4MFrames(path, dev, frames=n)
            wr = yuv.Y4MWriter(os.path.join(tmp, "alpha.y4m"), dev, W, H, kind="mono") if sink else None
            res = run_video_matte(m, src, trimap=tri, frames_are_rgb=True, device=dev, keep_on_device=True,
                                  on_frame=(lambda i, a, u8, out: wr.put(i, u8)) if sink else None)
            if wr is not None:
                wr.close()
            src.close()
            return res

        routes = dict(png=png, y4m=y4m, y4m_in=lambda n: y4m(n, False),
                      device=lambda n: run_video_matte(m, dclip[:n], trimap=tri, frames_are_rgb=True, device=dev, keep_on_device=True))
        first = {k: routes[k](min(T, 4))["alpha_u8"].cpu() for k in routes}               # plans each form once, untimed
        same = {k: bool(torch.equal(first[k][:min(4, distinct)], first["png"][:min(4, distinct)])) for k in routes}
        fps = {k: [] for k in routes}
        for _ in range(reps):
            for k in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                routes[k](T)
                torch.cuda.synchronize()
                fps[k].append(T / (time.perf_counter() - t0))
        sizes = dict(y4m_frame_bytes=yuv.frame_bytes(H, W, "420p"), rgb_frame_bytes=H * W * 3,
                     png_bytes_mean=float(np.mean([os.path.getsize(p) for p in set(pngs)])))
    return fps, same, sizes


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--clip-frames", type=int, default=120)
    ap.add_argument("--distinct", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_bench.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "yuv_bench measures on the GPU; there is no other way to get these numbers"
    lines = ["# Video streams: otvm_yuv_to_rgb / otvm_rgb_to_yuv420 and the Y4M route", "",
             "`python tools/yuv_bench.py --iters %d --clip-frames %d --distinct %d --reps %d` on %s." % (
                 args.iters, args.clip_frames, args.distinct, args.reps, torch.cuda.get_device_name(0)), "",
             "## Kernels", "",
             "Median of %d calls between device events, microseconds; MB = bytes read + written.  `luma` (`otvm_luma_u8`, 4 B a pixel) and "
             "`crop` (`otvm_roi_crop` of the whole frame, 6 B a pixel) are the scale for one streaming pass." % args.iters, "",
             "| size | " + " | ".join("to_rgb %s" % l for l, _ in KERNEL_LAYOUTS) + " | to_yuv420 | luma | crop |",
             "|---|" + "---|" * (len(KERNEL_LAYOUTS) + 3)]
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        r = bench_kernels(H, W, args.iters)
        rows.append(r)
        print(json.dumps(r), flush=True)
        cell = lambda k: "%.1f us (%.1f MB, %.0f GB/s)" % (r[k + "_us"], r[k + "_mb"], r[k + "_mb"] / r[k + "_us"] * 1e3)
        lines.append("| %dx%d | " % (W, H) + " | ".join(cell("to_rgb_" + l) for l, _ in KERNEL_LAYOUTS) + " | %s | %s | %s |" % (
            cell("to_yuv420"), cell("luma"), cell("crop")))
    lines += ["", "A call of 8 - 20 us between two events is a launch as much as a transfer: the frames fit the last-level cache and the event pair carries the launch gap, so the GB/s column says how little of the time is memory, not how fast the kernel streams."]
    doc = dict(rows=rows)
    if args.clip_frames:
        fps, same, sizes = bench_clip(args.clip_frames, args.distinct, args.reps)
        doc.update(fps=fps, same=same, sizes=sizes)
        print(json.dumps(dict(fps=fps, same=same, sizes=sizes)), flush=True)
        lines += ["", "## Clip: 1920x1080, %d frames (%d distinct, played forward and backward), frames/s including IO" % (
            args.clip_frames, args.distinct), "",
            "One process, one model, one set of convolution configurations, the routes alternating, %d runs each; the host clock around "
            "work that ends in a device synchronise and closed writers.  A Y4M frame is %d bytes, its RGB form %d, a PNG of these "
            "(smooth, synthetic) frames %.0f on average." % (args.reps, sizes["y4m_frame_bytes"], sizes["rgb_frame_bytes"], sizes["png_bytes_mean"]), "",
            "| route | runs (frames/s) | median | first frames' alpha_u8 equal to png's |", "|---|---|---|---|"]
        names = dict(png="png: run_video_matte_io, PNG files in, PNG files out (the parent's route)",
                     y4m="y4m: Y4MFrames in, Y4MWriter(mono) out", y4m_in="y4m_in: Y4MFrames in, no sink",
                     device="device: frames resident on the device, no sink")
        for k in fps:
            lines.append("| %s | %s | %.2f | %s |" % (names[k], ", ".join("%.2f" % v for v in fps[k]), med(fps[k]), same[k]))
        gap = med(fps["device"]) - med(fps["png"])
        closed = med(fps["y4m"]) - med(fps["png"])
        lines += ["", "The gap between the PNG route and the device-only rate is %.2f frames/s here; the Y4M route recovers %.2f of it "
                  "(%.0f %%).  The source alone (`y4m_in`) runs at %.2f against the device's %.2f: %s" % (
                      gap, closed, 100.0 * closed / gap if gap > 0 else float("nan"), med(fps["y4m_in"]), med(fps["device"]),
                      "the upload and the conversion on the copy stream do not show on the frame."
                      if med(fps["y4m_in"]) >= 0.99 * med(fps["device"]) else
                      "the upload and the conversion on the copy stream show on the frame -- the launch stream's first kernel of a "
                      "frame waits for the event behind them.")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
        json.dump(doc, f, indent=1)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
