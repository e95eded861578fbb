"""Price of keyframe trimaps on one clip:

    python tools/keyframes_bench.py [--size 1080x1920] [--frames 100] [--reps 3] [--skip 10] [--max-num 5] [--json out.json]

One synthetic clip matted by run_video_matte with the trimap on frame 0 ({0}: the reference's schedule), on frames 0 and T/2
({0, T/2}: one extra anchor) and on frame T/2 alone ({T/2}: forward, then backward sweep); the three alternate, --reps each,
in one process (one set of convolution configurations).  Per case: frames/s (wall time of the whole call, synchronised; best
and median of the repetitions) and the histogram of the memory read's T_read over the clip's frames.  Also the label pass alone
(otvm_trimap_apply_labels on an empty, a 5 % and a full map; median of 30 launches between two events)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-num", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from otvm_amd import helpers, lib as L
    from otvm_amd.engine import pad_amounts
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    H, W = (int(v) for v in args.size.split("x"))
    T = args.frames
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    frames, tri = synthetic_clip(H, W, T, seed=5)
    frames = [torch.from_numpy(f).cuda() for f in frames]          # resident: the clip's upload is not what is measured
    mid = T // 2
    tri_mid = np.ascontiguousarray(np.roll(tri, (mid // 2, mid), axis=(1, 2)))
    cases = {"{0}": {0: tri}, "{0,%d}" % mid: {0: tri, mid: tri_mid}, "{%d}" % mid: {mid: tri_mid}}
    run_video_matte(m, frames[:4], keyframes={0: tri, 2: tri}, skip=args.skip, max_num=args.max_num, keep_on_device=True)   # plans, tuning
    rows = {k: dict(fps=[], t_read=None) for k in cases}
    for rep in range(args.reps):
        for name, kf in cases.items():
            hist = {}

            def on_frame(i, alpha, u8, out):
                n = m._engine.last_T_read
                hist[n] = hist.get(n, 0) + 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_video_matte(m, frames, keyframes=kf, skip=args.skip, max_num=args.max_num, keep_on_device=True, on_frame=on_frame)
            torch.cuda.synchronize()
            rows[name]["fps"].append(T / (time.perf_counter() - t0))
            rows[name]["t_read"] = {str(k): hist[k] for k in sorted(hist)}
    for name, r in rows.items():
        f = sorted(r["fps"])
        r["fps_best"], r["fps_median"] = f[-1], f[len(f) // 2]
        print("%-8s frames/s best %.2f median %.2f (%s) | T_read histogram %s"
              % (name, r["fps_best"], r["fps_median"], ", ".join("%.2f" % v for v in r["fps"]), r["t_read"]))
    # the label pass alone
    lib = L.load()
    lw, uw, lh, uh = pad_amounts(H, W, 32)
    Hp, Wp = H + lh + uh, W + lw + uw
    probs = torch.rand(3 * Hp * Wp, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.Generator(np.random.PCG64(0))
    label_us = {}
    for name, dens in (("empty", 0.0), ("5pct", 0.05), ("full", 1.0)):
        lab = np.full((H, W), 255, np.uint8)
        has = rng.random((H, W)) < dens
        lab[has] = rng.integers(0, 3, int(has.sum()), dtype=np.uint8)
        ld = torch.from_numpy(lab).cuda()
        call = lambda: L.check(lib.otvm_trimap_apply_labels(probs.data_ptr(), ld.data_ptr(), H, W, Hp, Wp, lh, lw, st))
        for _ in range(3):
            call()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(60)]
        for i in range(30):
            ev[2 * i].record()
            call()
            ev[2 * i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(30))
        label_us[name] = 1e3 * ms[15]
        print("otvm_trimap_apply_labels %dx%d %-5s: %.1f us" % (W, H, name, label_us[name]))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(dict(size=[H, W], frames=T, skip=args.skip, max_num=args.max_num, cases=rows, label_pass_us=label_us),
                  open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
