#!/usr/bin/env python
"""bench.py -- OTVM per-frame inference throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A step = one frame of the hot path (EvalModel.forward: trimap propagation + alpha prediction + memorize)
on a synthetic 1920x1080 clip (BASELINE.json configs[2]: T=100, memory every 5 frames, max 5 slots).
The clip is ALWAYS BASELINE's length (100 frames at 1080p, 50 at 832x480, 200 at 4K; --clip-frames overrides): when
warmup + steps is shorter, the clip's first frames run as an untimed lead-in and the LAST `steps` frames are timed, so the timed
frames read a full bank (5 slots) whatever --steps says (eval.py:157-189: the loop and its memorize schedule).
Frames are resident in HBM as fp32 BGR [1,1,3,H,W] tensors (the reference DataLoader's format) before
the timed region starts.  One process per GPU; with N>1 every rank mattes its own sequence (sequences
are independent, frames inside a sequence are strictly sequential -- SURVEY.md 8e), no data-path
collective; ranks meet in one all-reduce for the timing/metric sums.  value = total frames / max time.

A plain run sets up, runs the lead-in and warm-up, times the steps, writes the outputs of the last timed step (--dump-outputs)
and prints the result line.  Extra legs, only with --full (rank 0, N=1): `roofline` (all convolution launches of the plan:
algorithmic FLOPs / HIP-event time per launch, instrumented replay of the timed frames on the same stream; `traffic` = HBM-side
bytes per launch from two short child runs of this script under `rocprofv3 --pmc`, live_traffic), `cpu_baseline` (the CPU oracle
timed on the host cores for one steady-state frame of the same clip) and, with --precision f16, `alpha_error_vs_f16x3`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# MI355X_MICROARCH.md, dense peaks.  f16x3 issues three f16 MFMAs per fp32-equivalent product, so its
# roofline for ALGORITHMIC (fp32-equivalent) FLOPs is the f16 peak / 3.
# "f16" (labelled reduced-precision mode, never the default): one MFMA pass per product in the implicit-GEMM and patch kernels,
# priced against the plain f16 peak
PEAK_TFLOPS = {"f32": 157.3, "f16x3": 2500.0 / 3.0, "f16": 2500.0}
POWER_LIMITED_PEAK = {"f16x3": 1650.0 / 3.0, "f16": 1650.0}       # tools/probes/mfma_probe.hip, random hi/lo operands, 256 CUs: 1598 - 1710 TFLOP/s f16 over four
                                                    # boxes (profiles/r02_mfma_power_ceiling.txt: 1659)
KERNEL_NAME = {"f32": "all otvm_conv2d launches: conv_igemm_f32_kernel (v_mfma_f32_32x32x2_f32)",
               "f16x3": "all convolution launches of the plan: conv_igemm_f16x3_kernel + conv_patch_f16x3_kernel + conv_stem_f16x3_kernel "
                        "(+ split-K finish) + stm_bottleneck_f16x3_kernel (three / four fused convolutions of an STM res2 block); "
                        "three f16 MFMA passes per fp32-equivalent MAC (v_mfma_f32_16x16x32_f16 in the LDS-DMA implicit-GEMM and nine-tap patch tiles, "
                        "v_mfma_f32_32x32x16_f16 elsewhere)",
               "f16": "the same launches in the single-pass mode: conv_igemm_f16x3_kernel<..., NPASS = 1> and conv_patch_f16x3_kernel<..., "
                      "NPASS = 1> issue ONE v_mfma_f32_32x32x16_f16 per MAC on fp16-rounded operands; the stem, 16-wide head, fused STM "
                      "bottleneck and memory-read kernels keep three passes (priced as if single-pass: frac is a lower bound)"}
DTYPE_NAME = {"f32": "f32", "f16x3": "f16x3 (fp32 operands split into fp16 hi+lo, fp32 accumulate)",
              "f16": "f16 (fp32 accumulate) -- REDUCED PRECISION, labelled mode: not the parity-graded configuration"}


CONV_KERNELS = ("conv_igemm", "conv_patch", "conv_stem", "conv_head", "conv_wave", "stm_bottleneck", "splitk_finish")   # what the plan counts as a conv launch
MEMREAD_KERNELS = ("memory_read_f16x3_kernel", "memory_read_combine", "memory_read_kernel")
BASELINE_CLIP = {(1080, 1920): 100, (480, 832): 50, (2160, 3840): 200}      # BASELINE.json configs[2], [1], [4]: frames per clip


def sum_conv_counter(csv_path, counter, kernels=CONV_KERNELS):
    """(sum of Counter_Value, rows) over the rows of the kernels named in `kernels` (default: the convolution kernels) of one
    rocprofv3 counter_collection.csv"""
    import csv
    tot, rows = 0.0, 0
    with open(csv_path) as fh:
        for row in csv.DictReader(fh):
            if row["Counter_Name"] == counter and any(t in row["Kernel_Name"] for t in kernels):
                tot += float(row["Counter_Value"])
                rows += 1
    return tot, rows


def child_line(stdout):
    """The JSON line a child run of this script printed (rocprofv3 writes around it)."""
    for ln in reversed(stdout.splitlines()):
        ln = ln.strip()
        if ln.startswith('{"metric"'):
            return json.loads(ln)
    return None


def live_traffic(H, W, extra_args=(), kernels=CONV_KERNELS, calls_key="conv_calls_total", clip=11, steps=8, warmup=3, timeout_s=100):
    """HBM-side bytes per launch of THIS tree on THIS box: two child runs of this script (a `clip`-frame clip, the parent's tuned
    configurations) under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` with --kernel-trace only, in separate passes as
    MI355X_MICROARCH.md prescribes; KiB -> bytes, FETCH_SIZE x 2 (gfx950) -- the arithmetic of tools/pmc_traffic.py.
    The divisor is the CHILD's own count of launches (its JSON line's `calls_key`: every otvm_conv2d / fused-bottleneck / head-conv
    call of that process, first frame and tuner launches included), so bytes and launches cover the same frames.
    Returns (bytes per launch, description, child line) or (None, reason, None)."""
    import glob
    import shutil
    import subprocess
    import tempfile
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rp):
        return None, "rocprofv3 not found", None
    tmp = tempfile.mkdtemp(prefix="otvm_pmc_", dir="/tmp")
    try:
        from otvm_amd import engine as E
        tune = os.path.join(tmp, "tune.json")
        keep = E.TUNE_FILE
        E.TUNE_FILE = tune
        try:
            E._save_tune_file()                                  # the children run the configurations this process timed
        finally:
            E.TUNE_FILE = keep
        env = dict(os.environ, TMPDIR="/tmp", OTVM_TUNE_FILE=tune)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--clip-frames", str(clip),
               "--height", str(H), "--width", str(W), "--no-cpu-baseline", "--no-roofline"] + list(extra_args)
        kib, calls, line = {}, None, None
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            r = subprocess.run([rp, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--"] + cmd,
                               cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            files = glob.glob(d + "/**/*counter_collection.csv", recursive=True)
            if r.returncode != 0 or not files:
                return None, "rocprofv3 --pmc %s: rc %d, %d counter files" % (counter, r.returncode, len(files)), None
            tot, rows = sum_conv_counter(files[0], counter, kernels)
            if rows == 0:
                return None, "no %s rows for the kernels %s" % (counter, "/".join(kernels)), None
            kib[counter] = tot
            line = child_line(r.stdout)
            if line is None or not line.get(calls_key):
                return None, "the child run printed no %s" % calls_key, None
            if calls is not None and calls != line[calls_key]:
                return None, "the two child runs issued different launch counts (%s vs %s)" % (calls, line[calls_key]), None
            calls = line[calls_key]
        total = (2.0 * kib["FETCH_SIZE"] + kib["WRITE_SIZE"]) * 1024.0
        return total / calls, ("live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate child runs of this command on a %d-frame "
                               "clip, --kernel-trace only; KiB -> bytes, FETCH_SIZE x 2 on gfx950), %.2f GB over the %d launches the "
                               "child itself issued (its first frame included on both sides)" % (clip, total / 1e9, calls)), line
    except Exception as e:                                       # (a timeout, a missing tool, an unreadable file: the committed value stays)
        return None, repr(e)[:200], None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def clip_plan(H, W, steps, warmup, clip_frames=0):
    """(frames of the clip, untimed lead-in frames): BASELINE's clip length for the resolution (or `clip_frames`), never fewer than
    warmup + steps; frames [0, lead_in) are the lead-in, [lead_in, lead_in + warmup) the warm-up, the LAST `steps` frames are
    timed -- so the driver's `--steps 20 --warmup 5` times frames 80 .. 99 of the 100-frame clip (it used to matte a
    25-frame clip whose timed frames read 2 - 5 slots)."""
    T = max(clip_frames if clip_frames > 0 else BASELINE_CLIP.get((H, W), 0), warmup + steps)
    return T, T - warmup - steps


def device_clip(H, W, T, seed, dev):
    """Smooth random video generated on the device (synthetic-data plumbing, not the measured path):
    bilinear-upsampled low-res noise with per-frame drift + a moving disc; uint8-quantised BGR as fp32."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    h, w = H // 8, W // 8
    base = torch.rand(1, 3, h, w, generator=g).to(dev)
    drift = (torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    frames = []
    for t in range(T):
        lo = (base + 0.02 * t * drift).clamp(0, 1)
        img = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)
        disc = ((yy - (H / 2 + 0.5 * t)) ** 2 + (xx - (W / 2 + 1.0 * t)) ** 2) < (H / 4) ** 2
        img = torch.where(disc[None, None], 0.35 + 0.65 * img, 0.75 * img)
        frames.append(torch.floor(img * 255.0 + 0.5).clamp(0, 255)[None].contiguous())   # [1,1,3,H,W]
    return frames


def build_model(dev, dilate_kernel=12, precision=None):
    from otvm_amd import helpers
    from otvm_amd.synth_weights import synthetic_state_dict
    sd = synthetic_state_dict(0)
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", dilate_kernel), "Test", dilate_kernel)
    m.load_state_dict(sd, strict=True)
    m.precision = precision
    return m.to(dev).eval(), sd


def frame_kwargs(t, T, skip, max_num, stress_bank=False):
    if stress_bank:
        # BASELINE configs[4] as written ("mem-every-1, growing KV bank"): every frame is memorised and nothing is evicted.
        # The reference's own rule turns `skip <= 2` into memorize=False (eval.py:188-189) and caps the bank at
        # MEMORY_MAX_NUM, so this is a stress knob of the build (max_memory_num = T), not reference semantics.
        return dict(first_frame=(t == 0), last_frame=(t == T - 1), memorize=True, max_memory_num=T)
    return dict(first_frame=(t == 0), last_frame=(t == T - 1), memorize=(t % skip == 0) if skip > 2 else False,
                max_memory_num=max_num)


OUTPUT_NAMES = ("scaled_imgs", "preds_trimap", "tri_gt", "preds_alpha", "scaled_gts")   # EvalModel.forward's 5-tuple
DUMP_BUDGET = 64 * 10 ** 6 - (1 << 16)  # bytes of the arrays of --dump-outputs together (64 MB, room left for the .npy headers)
DUMP_SAMPLE = 1 << 20                   # values kept of an output written as a sample


def dump_plan(shapes, budget=DUMP_BUDGET, sample=DUMP_SAMPLE):
    """[(name, whole)] for the (name, shape) pairs, in order: an output is written whole (float32) when it fits the budget with a
    sample's room left for every output after it, otherwise as `sample` values at fixed positions (dump_outputs)."""
    plan, used = [], 0
    for i, (name, shape) in enumerate(shapes):
        n = int(np.prod(shape))
        rest = sum(min(int(np.prod(s)), sample) for _, s in shapes[i + 1:]) * 4
        whole = n <= sample or used + 4 * n + rest <= budget
        used += 4 * (n if whole else sample)
        plan.append((name, whole))
    return plan


def dump_outputs(out_dir, outs):
    """What the last timed step returned -- one EvalModel.forward 5-tuple per sequence -- as out_dir/<name>.npy, float32.  Alpha and
    trimap first, so they are the ones written whole; an output too large for the budget is written as <name>_sample.npy: the
    values at DUMP_SAMPLE positions of its flattened array drawn by numpy's default_rng(0), the same positions for the same shape
    in every run.  With --batch B > 1 the names carry the sequence: seq<b>_<name>.
    The inputs are the same in every run; the kernel configurations are not: each process times them at plan time, and two runs
    that chose differently part well beyond rounding over the 100-frame clip (1080p: a tenth of the alpha values by > 1e-3).  For
    output-by-output comparisons give both runs one OTVM_TUNE_FILE (the first saves its choices, the next loads them: bit-identical
    dumps)."""
    os.makedirs(out_dir, exist_ok=True)
    pre = (lambda b: "") if len(outs) == 1 else (lambda b: "seq%d_" % b)
    order = ("preds_alpha", "preds_trimap", "scaled_imgs", "tri_gt", "scaled_gts")
    arrays = [(pre(b) + k, o[OUTPUT_NAMES.index(k)]) for k in order for b, o in enumerate(outs)]
    for (name, x), (_, whole) in zip(arrays, dump_plan([(n, tuple(x.shape)) for n, x in arrays])):
        v = x.detach().float().cpu().numpy()
        if not whole:
            idx = np.sort(np.random.default_rng(0).choice(v.size, DUMP_SAMPLE, replace=False))
            v, name = v.reshape(-1)[idx], name + "_sample"
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(v, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=80)        # (with BASELINE's 100-frame clip: 15 lead-in + 5 warm-up frames in front,
    ap.add_argument("--warmup", type=int, default=5)        #  every timed frame reads the full five-slot bank)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--clip-frames", type=int, default=0,
                    help="frames of the clip (default: BASELINE's -- 100 at 1920x1080, 50 at 832x480, 200 at 3840x2160 -- and never "
                         "fewer than warmup + steps); the LAST `steps` frames are timed, the frames in front of warmup are an untimed lead-in")
    ap.add_argument("--skip", type=int, default=5)
    ap.add_argument("--max-num", type=int, default=5)
    ap.add_argument("--precision", default=None, choices=["f32", "f16x3", "f16"],
                    help="conv arithmetic: f16x3 = split-fp16 MFMA with fp32-class accuracy (default), f32 = exact-fp32 MFMA, "
                         "f16 = ONE fp16 MFMA pass (reduced precision, reported with its alpha error against f16x3; never the headline)")
    ap.add_argument("--layer-report", default=None, help="write the per-layer conv timing table (JSON) to this path")
    ap.add_argument("--tune-report", default=None, help="write the plan-time autotuner's choices (JSON) to this path")
    ap.add_argument("--batch", type=int, default=1,
                    help="sequences stepped in lock-step per GPU (one launch per layer over the B images, per-sequence banks); "
                         "value then counts the frames of all of them.  The BASELINE headline is --batch 1")
    ap.add_argument("--stress-bank", action="store_true",
                    help="BASELINE configs[4] stress variant: memorise EVERY frame, never evict (max_memory_num = T)")
    ap.add_argument("--per-frame-report", default=None,
                    help="write per-frame device time (HIP events between frames) and slots read (JSON) to this path")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (the 5-tuple of EvalModel.forward) as "
                         "DIR/<name>.npy, float32, at most 64 MB in all (dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run the extra legs after the headline: roofline (per-launch HIP events, live PMC traffic), CPU "
                         "baseline, the f16 mode's alpha error against f16x3")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline leg")
    args = ap.parse_args()
    if args.layer_report and not args.full:
        ap.error("--layer-report comes from the roofline leg: add --full")

    # --gpus N > 1 outside a torch.distributed launch: start the N ranks ourselves (one process per GPU, RCCL)
    from otvm_amd.dist import self_launch_command
    cmd = self_launch_command(args.gpus, os.environ, torch.cuda.device_count(), os.path.abspath(__file__), sys.argv[1:])
    if cmd is not None:
        import subprocess
        raise SystemExit(subprocess.call(cmd))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU fallback")
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist, affinity = None, None
    if world > 1 or all(k in os.environ for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")):   # launched by torch.distributed.run (also exercised with 1 rank)
        import torch.distributed as dist
        from otvm_amd.dist import init_process_group, pin_rank_affinity
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        init_process_group(dev, rank=rank, world_size=world)      # RCCL ("nccl"); OTVM_DIST_BACKEND=gloo for one-GPU rehearsals
        affinity = pin_rank_affinity(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))

    H, W, K, Wm = args.height, args.width, args.steps, args.warmup
    T, lead_in = clip_plan(H, W, K, Wm, args.clip_frames)
    from otvm_amd.synth_data import disc_trimap
    model, sd = build_model(dev, precision=args.precision)
    if dist is not None:
        # every rank launches rank 0's kernel configurations (identical fp32 summation orders on all ranks): rank 0 builds
        # and times its plan first, the others adopt its choices before building theirs
        from otvm_amd.engine import share_tune_cache
        if rank == 0:
            model._get_engine().plan(H, W, max(1, args.batch))     # (the tuner's signature carries the batch size)
            torch.cuda.synchronize(dev)
        share_tune_cache(0)
    NB = max(1, args.batch)
    clips = [device_clip(H, W, T, seed=2000 + rank + 100 * b, dev=dev) for b in range(NB)]
    frames = clips[0]
    tri = torch.from_numpy(disc_trimap(H, W))[None, None].to(dev)
    a = torch.ones(1, 1, 1, H, W, device=dev)

    t_read = {}                                             # frame -> memory slots its segment step read
    host_issue = [0.0, 0]                                   # seconds the host spent inside model() (launching), frames counted
    frame_ev = {}                                           # frame -> event recorded behind it (--per-frame-report)

    def fkw(t):
        return frame_kwargs(t, T, args.skip, args.max_num, args.stress_bank)

    def run_frames(t0, t1, sink=None):
        for t in range(t0, t1):
            # _inputs_ready: the clip is resident in HBM and complete before the timed region starts (the bench contract),
            # so the query encoder of frame t may start while frame t-1's alpha network is still executing
            h0 = time.perf_counter()
            if NB == 1:
                outs = [model(a, frames[t], frames[t], tri=None, tri_gt=tri, large_input=False, _inputs_ready=True, **fkw(t))]
            else:
                fr = [c[t] for c in clips]
                outs = model.forward_batch([a] * NB, fr, fr, [tri] * NB, large_input=False, _inputs_ready=True, **fkw(t))
            out = outs[0]
            if not (t == T - 1):          # (the clip's last frame ends with the range guard's synchronising read: not issue time)
                host_issue[0] += time.perf_counter() - h0
                host_issue[1] += 1
            t_read[t] = model._engine.last_T_read
            if args.per_frame_report:
                frame_ev[t] = torch.cuda.Event(enable_timing=True)
                frame_ev[t].record()
            if sink is not None:
                sink.append(out[3])
        return outs

    def sync_all():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(dev)

    # ---- lead-in + warm-up (first frame: plan build, allocations; then steady frames): untimed
    run_frames(0, lead_in + Wm)
    sync_all()
    host_issue[0], host_issue[1] = 0.0, 0
    t_start = time.perf_counter()
    last_outs = run_frames(lead_in + Wm, T)
    sync_all()
    elapsed = time.perf_counter() - t_start
    alpha_last = last_outs[0][3]
    host_issue_s = host_issue[0] * K / max(1, host_issue[1])
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_outs)

    per_rank = None
    if dist is not None:
        # per-rank view (diagnosis of a scaling run): each rank's own time and the host time it spent issuing launches
        from otvm_amd.dist import reduce_device
        rdev = reduce_device(dev)
        mine = torch.tensor([elapsed, host_issue_s, float(dev.index)], dtype=torch.float64, device=rdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [dict(rank=i, device=int(v[2]), seconds=float(v[0]), frames_per_sec=K / float(v[0]),
                         host_issue_ms_per_frame=1000.0 * float(v[1]) / K) for i, v in enumerate(allr)]
        tt = torch.tensor([elapsed], dtype=torch.float64, device=rdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0])
        frames_total = torch.tensor([float(K * NB), 1.0], dtype=torch.float64, device=rdev)
        dist.all_reduce(frames_total, op=dist.ReduceOp.SUM)
        total_frames, ranks_seen = float(frames_total[0]), int(frames_total[1])
    else:
        total_frames, ranks_seen = float(K * NB), 1
    if ranks_seen != args.gpus:
        raise SystemExit("bench.py: --gpus %d but %d rank(s) took part in the run" % (args.gpus, ranks_seen))

    eng = model._engine
    pl = eng.last_plan
    Hp, Wp, hw = pl.Hp, pl.Wp, pl.hw
    peak = PEAK_TFLOPS[eng.precision_name]
    # algorithmic FLOPs of the timed frames: convs 2.6195 MFLOP per padded pixel + the memory read
    # with the number of slots each frame ACTUALLY read (short clips spend their first 16 frames below 5 slots)
    timed_T = [t_read[t] for t in range(lead_in + Wm, T)]
    flops_frame = (2.6195e6 * Hp * Wp + 1280.0 * (sum(timed_T) / float(K)) * hw * hw) * NB     # per STEP (NB frames)
    hist = {}
    for n_ in timed_T:
        hist[str(n_)] = hist.get(str(n_), 0) + 1
    result = {
        "metric": "frames_per_sec", "value": total_frames / elapsed, "unit": "frames/s", "n_gpus": ranks_seen,
        "steps": K, "warmup": Wm, "ms_per_step": 1000.0 * elapsed / K, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": DTYPE_NAME[eng.precision_name],
        "data": "synthetic",
        "lead_in_frames": lead_in,
        "config": {"workload": ("synthetic %dx%d clip, T=%d frames (untimed lead-in %d + warmup %d + timed: the last %d), %s, "
                                "trimap propagation + alpha + memorize per frame, one sequence per GPU" %
                                (W, H, T, lead_in, Wm, K, "EVERY frame memorised, no eviction (growing bank: build stress knob, "
                                 "BASELINE configs[4])" if args.stress_bank else
                                 "memory every %d, max %d slots" % (args.skip, args.max_num))),
                   "padded": [Hp, Wp], "weights": "synthetic (otvm_amd.synth_weights seed 0)",
                   "parallelism": "sequence-per-gpu x%d" % world if NB == 1 else "%d sequences in lock-step per gpu x%d gpus" % (NB, world),
                   "batch": NB,
                   "T_read_timed_frames": {"mean": sum(timed_T) / float(K), "histogram": hist}},
        "ranks_seen": ranks_seen,
        # the collectives of this run (rank count, max time, per-rank gather, tune-cache broadcast) ran on this backend;
        # "nccl" = RCCL; None = plain process, no process group
        "dist_backend": None if dist is None else dist.get_backend(),
        # wall time the host spends inside model() per step: issue time when the launch lists are replayed as graphs; with
        # direct launches the HIP queue fills up and the host blocks in launches, so this approaches ms_per_step
        "host_issue_ms_per_frame": 1000.0 * host_issue_s / K,
        "graphs": bool(__import__("otvm_amd.engine", fromlist=["graphs_wanted"]).graphs_wanted(model._engine.use_graphs, Hp * Wp)),
        "algorithmic_tflop_per_frame": flops_frame / 1e12,
        "achieved_tflops_whole_frame": flops_frame / 1e12 / (elapsed / K),
        "alpha_checksum": float(alpha_last.double().mean()),
        # launches this process issued so far (lead-in, warm-up and timed frames, tuner launches): what a parent run divides this
        # run's PMC byte counts by (live_traffic)
        "conv_calls_total": int(model._engine.conv_calls),
        "memory_read_calls_total": int(sum(1 for t in t_read.values() if t > 0) * NB),
        "memory_read_slots_total": int(sum(t_read.values()) * NB),
    }

    if per_rank is not None:
        result["per_rank"] = per_rank
        result["cpu_affinity_rank0"] = affinity
    if args.per_frame_report and rank == 0:
        ts = sorted(frame_ev)
        rows = [dict(frame=t, slots_read=t_read[t], ms=frame_ev[ts[i - 1]].elapsed_time(frame_ev[t]))
                for i, t in enumerate(ts) if i > 0 and t >= lead_in + Wm]
        json.dump(dict(workload=result["config"]["workload"], padded=[Hp, Wp], hw=hw, frames=rows), open(args.per_frame_report, "w"), indent=0)

    if rank == 0 and args.full and not args.no_roofline:          # (N > 1: the other ranks wait in the final barrier)
        # instrumented replay of a window of steady-state frames: HIP events around each conv launch
        nrep = min(K, 10)
        eng.prof = []
        run_frames(T - nrep, T)
        torch.cuda.synchronize(dev)
        prof_all, eng.prof = eng.prof, None
        prof = [p_ for p_ in prof_all if p_[0].startswith("conv ")]
        mr = [p_ for p_ in prof_all if p_[0] == "memory_read"]
        tot_ms = sum(e0.elapsed_time(e1) for _, _, e0, e1, _ in prof)
        tot_fl = float(sum(f for _, f, _, _, _ in prof))
        tot_by = float(sum(b for _, _, _, _, b in prof))
        n = len(prof)
        per_layer = {}
        for label, f, e0, e1, by in prof:
            d = per_layer.setdefault(label, [0.0, 0.0, 0, 0.0])
            d[0] += e0.elapsed_time(e1); d[1] += f; d[2] += 1; d[3] += by
        worst = sorted(per_layer.items(), key=lambda kv: -kv[1][0])[:8]
        if args.layer_report:
            rows = [dict(layer=k, ms_per_frame=v[0] / nrep, gflop_per_frame=v[1] / nrep / 1e9, launches_per_frame=v[2] / nrep,
                         tflops=v[1] / (v[0] * 1e-3) / 1e12, gbyte_per_frame=v[3] / nrep / 1e9,
                         tbyte_per_s=v[3] / (v[0] * 1e-3) / 1e12) for k, v in sorted(per_layer.items(), key=lambda kv: -kv[1][0])]
            json.dump(rows, open(args.layer_report, "w"), indent=0)
        achieved = tot_fl / (tot_ms * 1e-3) / 1e12
        # HBM bytes per conv launch from the committed PMC passes of this same command (profiles/, tools/pmc_traffic.py);
        # only quoted when that run matches this configuration
        traffic = None
        import glob
        tpaths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_conv_traffic_%s_%dx%d.json" % (eng.precision_name, W, H))))
        if tpaths and args.batch <= 1:                      # the most recent round's passes (collected with one sequence per step)
            tj = json.load(open(tpaths[-1]))                # bytes of all conv kernels per frame / otvm_conv2d calls per frame
            traffic = tj["traffic_bytes_per_frame"] / (n / nrep) if "traffic_bytes_per_frame" in tj else tj.get("traffic_bytes_per_launch")
        traffic_source = None if traffic is None else "committed PMC passes of this command: profiles/" + os.path.basename(tpaths[-1])
        mr_ms = sum(e0.elapsed_time(e1) for _, _, e0, e1, _ in mr)
        mr_dominant = bool(mr) and mr_ms > tot_ms           # (the growing bank of configs[4]: the frame IS the memory read)
        default_cfg = (args.skip == 5 and args.max_num == 5 and not args.stress_bank and not args.per_frame_report)
        live_env = os.environ.get("OTVM_BENCH_LIVE_PMC")
        if (world == 1 and args.batch <= 1 and eng.precision_name == "f16x3" and default_cfg and not mr_dominant
                and (live_env or "1") != "0"):
            # live: this run's own FETCH_SIZE / WRITE_SIZE passes (two short child runs of this script under rocprofv3, after the
            # timed region); any failure keeps the committed value above and says so
            live, why, _ = live_traffic(H, W)
            if live is not None:
                traffic, traffic_source = live, why
            else:
                traffic_source = "%s (live PMC passes not available: %s)" % (traffic_source, why)
        conv_block = {
            "bound": "mfma", "kernel": KERNEL_NAME[eng.precision_name],
            "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            "traffic": traffic, "traffic_source": traffic_source,
            # what the matrix cores of this chip sustain under its power limit with realistic operand values and NO memory
            # traffic (tools/probes/mfma_probe.hip, profiles/r02_mfma_power_ceiling.txt): 1598 TFLOP/s f16 = 533 f16x3;
            # informative only, `frac` above is priced against the nominal peak
            "power_limited_peak": POWER_LIMITED_PEAK.get(eng.precision_name),
            "frac_of_power_limited_peak": (achieved / POWER_LIMITED_PEAK[eng.precision_name]
                                           if eng.precision_name in POWER_LIMITED_PEAK else None),
            "algorithmic_bytes_per_launch": tot_by / n,
            "launches_per_frame": n / nrep, "avg_launch_ms": tot_ms / n, "algorithmic_gflop_per_launch": tot_fl / n / 1e9,
            "conv_ms_per_frame": tot_ms / nrep, "conv_share_of_frame": (tot_ms / nrep) / (1000.0 * elapsed / K),
            "slowest_layers_ms_per_frame": {k: round(v[0] / nrep, 3) for k, v in worst},
            "method": "torch.cuda.Event pairs on the launch stream around every otvm_conv2d launch, replay of the last "
                      "%d timed frames; FLOPs = 2*Ho*Wo*Cout*kh*kw*Cin (un-padded)" % nrep,
        }
        mr_block = None
        if mr:
            # the memory-read contraction (north_star: >= 40 % MFMA utilisation): algorithmic FLOPs 1280*T*hw^2 over the
            # HIP-event time of otvm_memory_read_f16x3 (kernel + combine), same replay.  Algorithmic bytes of one read:
            # the bank's keys and values once (640 fp32-equivalent values per position and slot: the packed split-fp16 copy has the
            # same size), the query key in, the 512-channel readout out
            mr_fl = float(sum(f for _, f, _, _, _ in mr))
            mr_t = mr_fl / (mr_ms * 1e-3) / 1e12
            mr_T = [int(b) for _, _, _, _, b in mr]
            mr_block = {"bound": "mfma", "kernel": "memory_read_f16x3_kernel + memory_read_combine_kernel (STM.py:140-163: softmax(K^T q / sqrt(128)) "
                                                   "over the memory axis and the value readout, flash-style over the packed bank)",
                        "ms_per_launch": mr_ms / len(mr), "launches": len(mr), "achieved": mr_t, "peak": peak,
                        "unit": "TFLOP/s", "frac": mr_t / peak, "T_read": mr_T,
                        "algorithmic_bytes_per_launch": (640.0 * sum(mr_T) / len(mr_T) + 640.0) * hw * 4.0,
                        "traffic": None, "traffic_source": None,
                        "note": "frac = share of the MFMA peak spent on ALGORITHMIC flops (1280 * T * hw^2 per read); the kernel also "
                                "issues the softmax rescale and padded tiles, see profiles/ for MFMA-busy"}
            if mr_dominant and world == 1 and args.batch <= 1 and eng.precision_name == "f16x3" and live_env == "1":
                # opt-in (two more passes over the whole growing-bank clip under rocprofv3): HBM-side bytes per memory read
                xa = ["--skip", str(args.skip), "--max-num", str(args.max_num)] + (["--stress-bank"] if args.stress_bank else [])
                live, why, cl = live_traffic(H, W, extra_args=xa, kernels=MEMREAD_KERNELS, calls_key="memory_read_calls_total",
                                             clip=T, steps=K, warmup=Wm, timeout_s=900)
                mr_block["traffic"], mr_block["traffic_source"] = live, why
                if cl is not None:                            # the child's population: every read of the clip (T_read = 1 .. T - 1)
                    mr_block["traffic_population"] = {"reads": cl["memory_read_calls_total"], "mean_T_read": cl["memory_read_slots_total"] / float(cl["memory_read_calls_total"]),
                                                      "algorithmic_bytes_per_read": (640.0 * cl["memory_read_slots_total"] / cl["memory_read_calls_total"] + 640.0) * hw * 4.0}
        if mr_dominant:
            # the dominant kernel of this run is the memory read: `roofline` names it, the convolutions keep their block
            result["roofline"] = mr_block
            result["conv_roofline"] = conv_block
        else:
            result["roofline"] = conv_block
            if mr_block is not None:
                result["memory_read"] = mr_block

    if rank == 0 and args.full and world == 1 and NB == 1 and eng.precision_name == "f16":
        # the labelled single-pass mode reports what it costs in accuracy: the first frames of the same clip through an f16x3 model
        # (the parity-graded configuration) and through this one, alpha against alpha
        nerr = min(T, 26)
        got = []
        run_frames(0, nerr, sink=got)
        torch.cuda.synchronize(dev)
        got = [g_.clone() for g_ in got]
        m3, _ = build_model(dev, precision="f16x3")
        ref3 = []
        for t in range(nerr):
            ref3.append(m3(a, frames[t], frames[t], tri=None, tri_gt=tri, large_input=False, **fkw(t))[3].clone())
        torch.cuda.synchronize(dev)
        dmax = [float((g_ - r_).abs().max()) for g_, r_ in zip(got, ref3)]
        dmean = [float((g_ - r_).abs().mean()) for g_, r_ in zip(got, ref3)]
        sad = [float((g_ - r_).abs().sum()) / 1000.0 for g_, r_ in zip(got, ref3)]
        u8 = [float(((g_ * 255).floor() != (r_ * 255).floor()).float().mean()) for g_, r_ in zip(got, ref3)]
        result["alpha_error_vs_f16x3"] = {
            "frames": nerr, "max_abs": max(dmax), "max_abs_per_frame_median": sorted(dmax)[nerr // 2], "mean_abs": sum(dmean) / nerr,
            "sad_per_frame_mean": sum(sad) / nerr, "sad_unit": "sum |alpha - alpha_f16x3| / 1000 over the frame",
            "fraction_of_8bit_pixels_that_differ": sum(u8) / nerr, "finite": bool(all(torch.isfinite(g_).all() for g_ in got)),
            "note": "same clip, same weights, same memory schedule; the f16x3 run meets the 1e-3 contract against the reference "
                    "(tests/), this mode does not claim to"}
        del m3

    if rank == 0 and args.full and world == 1 and NB == 1 and not args.no_cpu_baseline:
        # CPU baseline: the oracle (port of the reference algorithm) on the host cores, ONE steady-state frame of the
        # same clip at full resolution; its bank is seeded from the device bank so no CPU warm-up frames are needed.
        from oracle.otvm_oracle import OtvmOracle
        orc = OtvmOracle(sd, dilate_kernel=12)
        t_s = 2
        # replay frames 0..t_s-1 on the device to obtain the bank state at frame t_s
        run_frames(0, t_s)
        eng.flush()
        torch.cuda.synchronize(dev)
        orc.bank = [(s["k"].t.reshape(hw, 128).t().reshape(128, Hp // 16, Wp // 16).cpu().contiguous(),
                     s["v"].t.reshape(hw, 512).t().reshape(512, Hp // 16, Wp // 16).cpu().contiguous(), s["frame"])
                    for s in eng.bank]
        fa, ff, ft = a.cpu(), frames[t_s].cpu(), tri.cpu()
        kw_s = fkw(t_s)
        bank_before, cap = list(orc.bank), {}
        c0 = time.perf_counter()
        ref = orc.frame(fa, ff, ff.clone(), tri_gt=ft, frame_id=t_s, capture=cap, **kw_s)
        cpu_s = time.perf_counter() - c0
        hip = model(a, frames[t_s], frames[t_s], tri=None, tri_gt=tri, **kw_s)
        torch.cuda.synchronize(dev)
        d_raw = float((hip[3].cpu() - ref[3]).abs().max())
        # same protocol as tests/test_gpu_fullsize.py: where the 3-class argmax feeding the distance transform differs,
        # the pixel must be a near-tie in the oracle, and the oracle frame is re-evaluated with the device's tie-breaks
        pl = eng.last_plan
        cls_h = pl.CLS.reshape(pl.Hp, pl.Wp).cpu().long()
        flips = cls_h != cap["cls"]
        ties, gap = int(flips.sum()), 0.0
        TIE_TOL = 2e-3                                      # the parity tests' near-tie bound (tests/test_gpu_fullsize.py)
        if ties:
            top2 = torch.sort(cap["tri_in"][0], dim=0, descending=True)[0]
            gap = float((top2[0] - top2[1])[flips].max())
            if gap <= TIE_TOL:
                orc.bank = bank_before
                ref = orc.frame(fa, ff, ff.clone(), tri_gt=ft, frame_id=t_s, class_override=cls_h, **kw_s)
            # else: a class flipped at a pixel that is NOT a near-tie in the oracle -- a genuine trimap / argmax error on the
            # device must not be aligned away: the raw difference stays the reported value
        diag = None
        if float((hip[3].cpu() - ref[3]).abs().max()) > 1e-3 or os.environ.get("OTVM_BENCH_FORCE_DIAG"):
            # should never happen (tests/ assert <= 1e-3 on this very flow): leave the per-stage differences in the record
            try:
                def nchw(act, cc=None):
                    cc = act.C if cc is None else cc
                    v = torch.as_strided(act.t, (act.H, act.W, cc), (act.W * act.ld, act.ld, 1), act.off)
                    return v.permute(2, 0, 1)[None].cpu().contiguous()

                def dd(got, want):
                    return [float((got - want).abs().max()), float(want.abs().max())]
                diag = {"x11": dd(nchw(pl.X11, 11), cap["x11"]), "l4": dd(nchw(pl.PPMCAT.ch(0, 2048)), cap["feats"][5]),
                        "x_dec": dd(nchw(pl.D80.ch(0, 70)), cap["x_dec"]), "k4": dd(nchw(pl.QK), cap["k4"]),
                        "m4": dd(nchw(pl.M4), cap["m4"]),
                        "tri_in": dd(pl.PROBS.reshape(1, 3, pl.Hp, pl.Wp).cpu(), cap["tri_in"]),
                        "alpha_p": dd(pl.ALPHA_P.reshape(1, 1, pl.Hp, pl.Wp).cpu(), cap["alpha_p"])}
            except Exception as e:                                  # diagnosis only
                diag = {"error": repr(e)}
        result["cpu_baseline"] = {
            "value": 1.0 / cpu_s, "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "1 steady-state frame (t=%d, segment + FBA + memorize, T_read=%d) of the same %dx%d clip; "
                      "oracle/otvm_oracle.py (PyTorch-CPU fp32, oneDNN) on %d threads of %d host cpus"
                      % (t_s, len(eng.bank), W, H, torch.get_num_threads(), os.cpu_count()),
            "seconds_per_frame": cpu_s,
            "alpha_maxabs_hip_vs_cpu_same_frame": float((hip[3].cpu() - ref[3]).abs().max()),
            "trimap_argmax_tie_breaks": ties, "tie_break_top2_gap_max": gap,
            "tie_breaks_aligned": bool(ties and gap <= TIE_TOL), "tie_gap_bound": TIE_TOL,
            "alpha_maxabs_before_tie_alignment": d_raw,
        }
        if diag is not None:
            result["cpu_baseline"]["stage_maxabs_and_range_on_mismatch"] = diag

    if rank == 0 and args.tune_report:
        from otvm_amd.engine import TUNE_LOG
        json.dump([dict(layer=n, shape=dict(H=sg[0], W=sg[1], Cin=sg[2], Cout=sg[4], k=sg[6], stride=sg[8], dil=sg[10]),
                        chosen=best, ms={str(k): round(v, 4) for k, v in ms.items()}) for n, sg, best, ms in TUNE_LOG],
                  open(args.tune_report, "w"), indent=0)
    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
