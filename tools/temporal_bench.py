"""Time the temporal stabilisation of alpha with device events:

    python tools/temporal_bench.py [--iters 30] [--sizes 480x832,1080x1920,2160x3840] [--clip-frames 24] [--reps 3] [--json out.json]

Per size (H x W), median of --iters calls, each between two events, three untimed calls first:
  luma   otvm_luma_u8 alone (3 B in, 1 B out per pixel)
  blend  otvm_temporal_blend alone, with a trimap at scale 1 and the byte output, on a flow of N(0, 3) pixels (every pixel
         gathers somewhere else: the worst case) and on a smooth flow (neighbouring pixels gather neighbouring taps)
  copy   a plain device copy (torch's copy_ of a uint8 buffer) of the blend's streamed byte count, 30 B per pixel in + out
         (alpha 4, flow 8, grey 1, trimap 12, out 4, byte 1): the yardstick for the two new kernels.  The blend's gathers (four
         taps of the previous alpha and grey plane per pixel, 20 B) are not in that count
  step   TemporalStabiliser.step: luma + otvm_optflow_farneback + blend + the allocation of the two fresh outputs
--clip-frames N: frames/s of run_video_matte(masks=...) on one synthetic 1920x1080 clip of N device-resident frames with and
without ``stabilise``, alternating, --reps each, one process (a same-box A/B).  Set OTVM_AUTOTUNE=0 or OTVM_TUNE_FILE so that every
run uses one set of convolution configurations."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fgr_bench import median_ms  # noqa: E402

STREAMED_BYTES = 4 + 8 + 1 + 12 + 4 + 1        # per pixel, in + out, with a trimap at scale 1
LUMA_BYTES = 3 + 1


def bench_size(H, W, iters):
    from otvm_amd import lib as L
    from otvm_amd.temporal import TemporalStabiliser
    lib = L.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(H * 7 + W)
    frames = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(2)]
    alpha = torch.rand((H, W), generator=g).to(dev)
    prev = torch.rand((H, W), generator=g).to(dev)
    flow = (torch.randn((H, W, 2), generator=g) * 3).to(dev)
    cls = torch.randint(0, 3, (H, W), generator=g)
    tri = torch.stack([cls == c for c in range(3)]).float().to(dev)
    grey = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    for f, gr in zip(frames, grey):
        L.check(lib.otvm_luma_u8(f.data_ptr(), H, W, 0, gr.data_ptr(), st), "luma_u8")
    out = torch.empty((H, W), device=dev)
    u8 = torch.empty((H, W), dtype=torch.uint8, device=dev)
    p = L.TemporalParams()
    p.H, p.W, p.alpha, p.prev, p.grey, p.grey_prev, p.flow = H, W, alpha.data_ptr(), prev.data_ptr(), grey[0].data_ptr(), grey[1].data_ptr(), flow.data_ptr()
    p.tri, p.th, p.tw, p.tri_scale = tri.data_ptr(), H, W, 1
    p.strength, p.inv_tau_colour, p.inv_tau_alpha = 0.5, 1.0 / 24.0, 2.0
    p.out, p.out_u8 = out.data_ptr(), u8.data_ptr()
    row = dict(H=H, W=W)
    row["luma_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_luma_u8(frames[0].data_ptr(), H, W, 0, grey[0].data_ptr(), st), "luma_u8"), iters)
    row["blend_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_temporal_blend(C.byref(p), st), "temporal_blend"), iters)
    # a smooth flow (what a moving subject gives): neighbouring pixels gather neighbouring taps
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([2.3 + 1.5 * torch.sin(yy / 97.0), -1.7 + 1.5 * torch.cos(xx / 131.0)], -1).contiguous().to(dev)
    p.flow = smooth.data_ptr()
    row["blend_smooth_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_temporal_blend(C.byref(p), st), "temporal_blend"), iters)
    p.flow = flow.data_ptr()
    n = H * W * STREAMED_BYTES
    src, dst = torch.empty(n // 2, dtype=torch.uint8, device=dev), torch.empty(n // 2, dtype=torch.uint8, device=dev)
    row["copy_us"] = 1e3 * median_ms(lambda: dst.copy_(src), iters)
    n = H * W * LUMA_BYTES
    src, dst = torch.empty(n // 2, dtype=torch.uint8, device=dev), torch.empty(n // 2, dtype=torch.uint8, device=dev)
    row["copy_luma_us"] = 1e3 * median_ms(lambda: dst.copy_(src), iters)
    stab = TemporalStabiliser(dev, H, W)
    stab.step(frames[0], alpha, trimap=tri)
    k = [0]

    def step():
        k[0] += 1
        stab.step(frames[k[0] & 1], alpha, trimap=tri)
    row["step_us"] = 1e3 * median_ms(step, iters)
    row["blend_mb"], row["luma_mb"] = H * W * STREAMED_BYTES / 1e6, H * W * LUMA_BYTES / 1e6
    row["blend_gbps"], row["luma_gbps"] = row["blend_mb"] / row["blend_us"] * 1e3, row["luma_mb"] / row["luma_us"] * 1e3
    row["copy_gbps"], row["copy_luma_gbps"] = row["blend_mb"] / row["copy_us"] * 1e3, row["luma_mb"] / row["copy_luma_us"] * 1e3
    return row


def bench_clip(frames, reps):
    from otvm_amd import helpers
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
    yy, xx = np.mgrid[0:H, 0:W]
    dmasks = []
    for t in range(frames):                                    # the clip's moving disc, a soft rim
        r = np.sqrt((yy - H / 2 - 0.5 * t) ** 2 + (xx - W / 2 - 1.0 * t) ** 2)
        dmasks.append(torch.from_numpy(np.floor(np.clip((H / 4 - r) / 6.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8)).cuda())
    routes = dict(plain=lambda n: run_video_matte(m, dclip[:n], masks=dmasks[:n], keep_on_device=True),
                  stabilise=lambda n: run_video_matte(m, dclip[:n], masks=dmasks[:n], keep_on_device=True, stabilise=True))
    for k in routes:                                           # plans each form once, untimed
        routes[k](min(frames, 3))
    fps = {k: [] for k in routes}
    for _ in range(reps):
        for k in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k](frames)
            torch.cuda.synchronize()
            fps[k].append(frames / (time.perf_counter() - t0))
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", default="480x832,1080x1920,2160x3840")
    ap.add_argument("--clip-frames", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        rows.append(bench_size(H, W, args.iters))
        print(json.dumps(rows[-1]), flush=True)
    print("| size | luma us | copy of 4 B/px us | blend us | blend, smooth flow us | copy of 30 B/px us | blend GB/s | copy GB/s | step us |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %dx%d | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f | %.0f | %.1f |" % (
            r["W"], r["H"], r["luma_us"], r["copy_luma_us"], r["blend_us"], r["blend_smooth_us"], r["copy_us"], r["blend_gbps"],
            r["copy_gbps"], r["step_us"]))
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        fps = bench_clip(args.clip_frames, args.reps)
        doc["clip_1080p_fps"] = fps
        print("run_video_matte(masks=...) 1920x1080, %d frames, alternating: %s" % (
            args.clip_frames, " | ".join("%s %s frames/s" % (k, ", ".join("%.2f" % v for v in vs)) for k, vs in fps.items())))
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
