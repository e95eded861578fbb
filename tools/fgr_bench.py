"""Time the foreground outputs with device events:

    python tools/fgr_bench.py [--iters 30] [--sizes 480x832,1080x1920,2160x3840] [--clip-frames 20] [--reps 3] [--json out.json]

Per size (H x W, padded to multiples of 32 as the engine pads): the refinement head's layer (3x3 conv 32 -> 16 + the head,
n_out 10, hidden state written, 16-wide tile) through otvm_conv2d_head and through otvm_conv2d_head_fgr, and otvm_fgr_outputs
with rgba only and with rgba + the composite over an image; median of --iters launches, each between two events.
--clip-frames N: frames/s of run_video_matte on one synthetic 1080p clip of N frames with the option off and on (RGBA + composite
over an image), alternating, --reps each, same process settings; set OTVM_TUNE_FILE so that every run uses one set of
convolution configurations."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    for i in range(iters):
        ev[2 * i].record()
        call()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
    return ms[len(ms) // 2]


def bench_size(H, W, iters):
    from otvm_amd import lib as L
    from otvm_amd.engine import Act, conv_params, pack_conv_weight, pad_amounts
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    dev = "cuda"
    lw, uw, lh, uh = pad_amounts(H, W, 32)
    Hp, Wp = H + lh + uh, W + lw + uw
    P = Hp * Wp
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(16, 32, 3, 3, generator=g) / math.sqrt(288)).to(dev)
    cw = pack_conv_weight(lib, dev, w, False, None, None, split=True, stream=st)
    bias = (torch.randn(16, generator=g) * 0.2).to(dev)
    hw, hb = (torch.randn(10, 16, generator=g) * 0.4).to(dev), (torch.randn(10, generator=g) * 0.3).to(dev)
    x = Act(torch.randn(P * 32, generator=g).to(dev), Hp, Wp, 32)
    img = Act(torch.rand(P * 4, generator=g).to(dev), Hp, Wp, 4)
    sm = Act(torch.zeros(P * 24, device=dev), Hp, Wp, 24)
    alpha, tri, fgr = torch.empty(P, device=dev), torch.empty(3 * P, device=dev), torch.empty(3 * P, device=dev)
    p = conv_params(x, cw, sm.ch(0, 16), bias, 1, 1, 1, 2, 0, None, L.PREC_F16X3)
    h = L.HeadParams()
    h.w, h.b, h.n_out, h.img, h.img_ld, h.P = hw.data_ptr(), hb.data_ptr(), 10, img.ptr, img.ld, P
    h.alpha_out, h.alpha_stride, h.tri_out = alpha.data_ptr(), 1, tri.data_ptr()
    h.sm, h.sm_ld = sm.ch(16, 8).ptr, sm.ld
    h.w16 = cw.w16.data_ptr()
    row = dict(H=H, W=W, Hp=Hp, Wp=Wp)
    row["head_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_conv2d_head(C.byref(p), C.byref(h), st)), iters)
    row["head_fgr_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_conv2d_head_fgr(C.byref(p), C.byref(h), fgr.data_ptr(), 0, st)), iters)
    row["head_us_again"] = 1e3 * median_ms(lambda: L.check(lib.otvm_conv2d_head(C.byref(p), C.byref(h), st)), iters)
    q = L.FgrParams()
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    comp = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    bg = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    q.alpha_p, q.fgr_p, q.rgba_u8 = alpha.data_ptr(), fgr.data_ptr(), rgba.data_ptr()
    q.Hp, q.Wp, q.H, q.W, q.lh, q.lw = Hp, Wp, H, W, lh, lw
    row["outputs_rgba_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_fgr_outputs(C.byref(q), st)), iters)
    q.comp_u8, q.bg_u8 = comp.data_ptr(), bg.data_ptr()
    row["outputs_rgba_comp_us"] = 1e3 * median_ms(lambda: L.check(lib.otvm_fgr_outputs(C.byref(q), st)), iters)
    # bytes moved by rgba + comp: alpha + 3 F planes read over the crop, background read, 4 + 3 bytes written
    row["outputs_rgba_comp_mb"] = H * W * (16 + 3 + 7) / 1e6
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
    clip, tri = synthetic_clip(H, W, frames, seed=7)
    dclip = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in clip]
    bg = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    kws = dict(off={}, on=dict(foreground=True, new_background=bg))
    for k in ("off", "on"):                                     # plans (and times) both forms once, untimed
        run_video_matte(m, dclip[:3], trimap=tri, keep_on_device=True, **kws[k])
    fps = dict(off=[], on=[])
    for _ in range(reps):
        for k in ("off", "on"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_video_matte(m, dclip, trimap=tri, keep_on_device=True, **kws[k])
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
    print("| size | head us | head + F us | head again us | outputs (rgba) us | outputs (rgba + comp over image) us | MB moved (rgba + comp) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %dx%d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (r["W"], r["H"], r["head_us"], r["head_fgr_us"], r["head_us_again"],
                                                                   r["outputs_rgba_us"], r["outputs_rgba_comp_us"], r["outputs_rgba_comp_mb"]))
    doc = dict(device=torch.cuda.get_device_name(0), rows=rows)
    if args.clip_frames:
        doc["clip_1080p_fps"] = fps = bench_clip(args.clip_frames, args.reps)
        print("run_video_matte 1080p, %d frames, alternating: off %s frames/s | on (rgba + comp) %s frames/s" % (
            args.clip_frames, ", ".join("%.2f" % v for v in fps["off"]), ", ".join("%.2f" % v for v in fps["on"])))
    if args.json:
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
