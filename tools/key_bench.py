"""Time the masks of keyed footage with device events and write profiles/key_trimap_bench.md:

    python tools/key_bench.py [--iters 30] [--sizes 1080x1920,2160x3840] [--clip-frames 24] [--reps 3] [--out profiles/key_trimap_bench.md]

Per size (H x W): the time per call -- the raw C call with a prebuilt parameter struct, median of --iters launches, each between
two events, output allocated once -- of
otvm_mask_from_chroma and of otvm_mask_from_plate at every radius, beside otvm_luma_u8 (a pass of the same size) and
otvm_trimap_from_mask (the step the keys feed), all measured in this run.
--clip-frames N: frames/s of run_video_matte on one synthetic 1920x1080 clip of N frames (a noisy green field, a moving disc)
through ``key=`` (chroma and plate) against ``masks=`` with the same masks precomputed and resident on the device; ONE process, the
routes alternating, --reps runs each.  Set OTVM_TUNE_FILE (or OTVM_AUTOTUNE=0) so that every run uses one set of convolution
configurations.  Only same-process comparisons mean anything: boxes differ by a few per cent."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fgr_bench import median_ms  # noqa: E402


def green_clip(H, W, T, seed=3):
    """(frames B, G, R; plate): a noisy green field with a moving soft-edged disc, the field again with fresh noise"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    field, disc = np.asarray((30, 200, 40), np.float32), np.asarray((200, 60, 90), np.float32)
    frames = []
    for t in range(T):
        r = np.sqrt((yy - H / 2 - 0.5 * t) ** 2 + (xx - W / 2 - 1.0 * t) ** 2).astype(np.float32)
        a = np.clip((H / 4 - r) / 6.0 + 0.5, 0, 1)[..., None]
        rgb = field * (1 - a) + disc * a + g.integers(-4, 5, (H, W, 3))
        frames.append(np.ascontiguousarray(np.clip(np.round(rgb), 0, 255).astype(np.uint8)[..., ::-1]))
    plate = np.clip(field[None, None] + g.integers(-4, 5, (H, W, 3)), 0, 255).astype(np.uint8)[..., ::-1]
    return frames, np.ascontiguousarray(plate)


def bench_calls(H, W, iters):
    """Like for like: every entry is the raw C call with its parameter struct built beforehand and its output allocated once --
    no wrapper, no allocation inside the timed region."""
    from otvm_amd import keys, lib as L
    from otvm_amd.masks import band_thresholds
    lib, dev = L.load(), torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    (frame,), plate = green_clip(H, W, 1)
    fd, pd = torch.from_numpy(frame).to(dev), torch.from_numpy(plate).to(dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    row = dict(H=H, W=W)
    k = keys.ChromaKey("green")
    cp = L.MaskFromChromaParams(frame=fd.data_ptr(), mask=out.data_ptr(), H=H, W=W, u8_rgb=0, kb=k.kb, kr=k.kr, qlo=k.qlo, qhi=k.qhi)
    row["chroma_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_mask_from_chroma(C.byref(cp), st), "chroma"), iters)
    for r in range(4):
        pp = L.MaskFromPlateParams(frame=fd.data_ptr(), plate=pd.data_ptr(), mask=out.data_ptr(), H=H, W=W, radius=r, lo=12, hi=40)
        row["plate_r%d_us" % r] = 1e3 * median_ms(lambda: L.check(lib.otvm_mask_from_plate(C.byref(pp), st), "plate"), iters)
    row["luma_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_luma_u8(fd.data_ptr(), H, W, 0, out.data_ptr(), st), "luma"), iters)
    mask = keys.key_mask(fd, k)
    t_fg, t_bg = band_thresholds(12)
    ws = torch.empty(lib.otvm_trimap_from_mask_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    tri = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    tp = L.MaskTrimapParams()
    tp.mask, tp.H, tp.W, tp.lo, tp.hi, tp.t_fg, tp.t_bg, tp.band_label, tp.trimap = mask.data_ptr(), H, W, 127, 128, t_fg, t_bg, 1, tri.data_ptr()
    row["trimap_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_trimap_from_mask(C.byref(tp), ws.data_ptr(), st), "trimap"), iters)
    row["chroma_mb"], row["plate_mb"] = H * W * 4 / 1e6, H * W * 7 / 1e6
    return row


def bench_clip(T, reps, skip, max_num):
    from otvm_amd import helpers, keys
    from otvm_amd.masks import Mask
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    frames, plate = green_clip(1080, 1920, T)
    dclip = [torch.from_numpy(f).cuda() for f in frames]
    ck, pk = keys.ChromaKey("green"), keys.PlateKey(plate)
    cm = [Mask(keys.key_mask(f, ck)) for f in dclip]
    pm = [Mask(keys.key_mask(f, pk)) for f in dclip]
    common = dict(keep_on_device=True, skip=skip, max_num=max_num)
    routes = {"key=ChromaKey": lambda n: run_video_matte(m, dclip[:n], key=ck, **common),
              "masks= (chroma masks resident)": lambda n: run_video_matte(m, dclip[:n], masks=cm[:n], **common),
              "key=PlateKey": lambda n: run_video_matte(m, dclip[:n], key=pk, **common),
              "masks= (plate masks resident)": lambda n: run_video_matte(m, dclip[:n], masks=pm[:n], **common)}
    for k in routes:                                           # plans (and times) form once, untimed
        routes[k](min(T, 3))
    fps = {k: [] for k in routes}
    for _ in range(reps):
        for k in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k](T)
            torch.cuda.synchronize()
            fps[k].append(T / (time.perf_counter() - t0))
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--clip-frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-num", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_trimap_bench.md"))
    args = ap.parse_args()
    lines = ["# Masks of keyed footage: time per call and frame rate of the route", "",
             "`tools/key_bench.py`, %s, one process; median of %d launches per entry, each between two device events." %
             (torch.cuda.get_device_name(0), args.iters), "",
             "| size | chroma key us | plate key r=0 us | r=1 | r=2 | r=3 | otvm_luma_u8 us | otvm_trimap_from_mask (r=12) us | chroma GB/s | plate r=1 GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        r = bench_calls(H, W, args.iters)
        lines.append("| %dx%d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f | %.0f |" % (
            W, H, r["chroma_us"], r["plate_r0_us"], r["plate_r1_us"], r["plate_r2_us"], r["plate_r3_us"], r["luma_us"], r["trimap_us"],
            r["chroma_mb"] / r["chroma_us"] * 1e3, r["plate_mb"] / r["plate_r1_us"] * 1e3))
        print(lines[-1], flush=True)
    lines += ["", "Bytes a call must move: 4 a pixel for the chroma key (3 in, 1 out), 7 for the plate key (the plate as well)."]
    if args.clip_frames:
        fps = bench_clip(args.clip_frames, args.reps, args.skip, args.max_num)
        lines += ["", "run_video_matte, synthetic 1920x1080 clip of %d frames resident on the device (a noisy green field, a moving disc), "
                  "routes alternating, %d runs each, frames/s:" % (args.clip_frames, args.reps), "", "| route | frames/s |", "|---|---|"]
        for k, v in fps.items():
            lines.append("| %s | %s |" % (k, ", ".join("%.2f" % x for x in v)))
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
