"""Print the launch lists of a plan, one line per step, in a form two builds of the engine can be compared by (diff):

    python tools/plan_dump.py [--height 96] [--width 128] [--batch 1] [--frames 0] [--out plan.txt]

Synthetic weights.  Per step: the list, the library symbol, the label, flops and bytes of a convolution, every argument.  Scalars as
they are; of a structure passed by reference every field; every pointer (which positional arguments are pointers: lib._PROTOS) as
the allocation it falls in + the byte offset -- a buffer of the plan, a packed weight, a state-dict tensor, a bank slot, the
GroupNorm statistics arena -- or ``ext`` (counted at the end).  Then upfold_routes, the tile of every fused-block parameter
block, n_gn, stats_bs.  --frames N mattes a clip of N frames first and lists the key / value steps of the bank slots as well.
The OTVM_* switches are read from the environment, as everywhere: one process per configuration."""
import argparse
import bisect
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fields(st):
    """(fn, args, label, flops, abytes) of a launch step."""
    return st.fn, st.args, st.label, st.flops, st.abytes


class Allocations:
    def __init__(self):
        self.spans, self.ext = {}, 0

    def add(self, name, t):
        if t is not None and torch.is_tensor(t) and t.numel():
            self.spans.setdefault(t.data_ptr(), (t.data_ptr() + t.numel() * t.element_size(), name))

    def freeze(self):
        self.starts = sorted(self.spans)

    def name(self, p):
        p = int(p or 0)
        if p == 0:
            return "null"
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0 and p < self.spans[self.starts[i]][0]:
            return "%s+%d" % (self.spans[self.starts[i]][1], p - self.starts[i])
        self.ext += 1
        return "ext"


def allocations(eng, plan, slots):
    from otvm_amd.engine import Act
    al = Allocations()
    for key, b in plan._bufs.items():
        al.add("buf%s" % (key,), b.t if isinstance(b, Act) else b)
    al.add("stats", plan.stats)
    for i, s in enumerate(slots):
        al.add("slot%d.k" % i, s["k"].t)
        al.add("slot%d.v" % i, s["v"].t)
    for name, cw in eng.W.items():
        for f in ("w", "w_hi", "w_lo", "w_scale", "w_frag", "w_wfrag", "w16", "bias"):
            al.add("W[%s].%s" % (name, f), getattr(cw, f))
    al.add("W_ppm", eng.W_ppm)
    for name, (mp, v) in eng.GP.items():
        al.add("GP[%s].Mp" % name, mp)
        al.add("GP[%s].v" % name, v)
    for name, t in eng.sd.items():
        al.add("sd[%s]" % name, t)
    al.freeze()
    return al


def fmt_value(v, ctype, al):
    if ctype is C.c_void_p:
        return al.name(v)
    if isinstance(v, C.Array):
        return "[" + ",".join(fmt_value(x, v._type_, al) for x in v) + "]"
    return repr(v)


def fmt_arg(a, argtype, al):
    obj = getattr(a, "_obj", None)                                # ctypes.byref(structure)
    if isinstance(obj, C.Structure):
        return "%s{%s}" % (type(obj).__name__, " ".join("%s=%s" % (n, fmt_value(getattr(obj, n), t, al)) for n, t in obj._fields_))
    if isinstance(a, C.Array):
        return fmt_value(a, None, al)
    return fmt_value(a, argtype, al)


def dump_steps(key, steps, al, out):
    from otvm_amd import lib as L
    tiles = []
    for st in steps:
        fn, args, label, flops, abytes = fields(st)
        argtypes = L._PROTOS[fn.__name__][1]
        out.append("%s | %s | %s | flops=%d abytes=%d | %s" % (key, fn.__name__, label, flops, abytes, " ; ".join(
            fmt_arg(a, t, al) for a, t in zip(args, argtypes))))
        for a in args:
            if isinstance(getattr(a, "_obj", None), L.StmBottleneckParams):
                tiles.append(a._obj.tile)
    return tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    from otvm_amd import helpers
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.synth_weights import synthetic_state_dict
    from otvm_amd.video import run_video_matte
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    m = m.cuda().eval()
    eng = m._get_engine()
    H, W = args.height, args.width
    if args.frames:
        frames, tri = synthetic_clip(H, W, args.frames, seed=5)
        run_video_matte(m, frames, trimap=tri, skip=2, max_num=3)
        torch.cuda.synchronize()
    plan = eng.plan(H, W, args.batch)
    slots = [s for s in list(eng.bank) + list(eng.free_slots) if s["plan"] is plan and "kv_steps" in s]
    al = allocations(eng, plan, slots)
    out, tiles = [], []
    for key, steps in plan.steps.items():
        tiles += dump_steps(key, steps, al, out)
    for i, s in enumerate(slots):
        dump_steps("slot%d.kv_steps" % i, s["kv_steps"], al, out)
    out.append("upfold_routes %r" % (sorted(plan.upfold_routes.items()),))
    out.append("fused-block tiles %r" % (tiles,))
    from otvm_amd.engine import TUNE_LOG
    out.append("n_gn %d stats_bs %d steps %d ext %d choices timed by this process %d"
               % (plan.n_gn, plan.stats_bs, sum(len(s) for s in plan.steps.values()), al.ext, len(TUNE_LOG)))
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
