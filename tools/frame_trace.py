"""Record what the engine's frame step issues, call by call, in a form two builds of otvm_amd/ can be compared by (diff):

    python tools/frame_trace.py [--root DIR] [--cases a,b,...] [--out trace.txt]

A companion to tools/plan_dump.py (which prints the launch lists a plan holds; this prints the order in which a frame call issues
them, to which stream, and the events that join the streams).  ``--root`` is the directory ``otvm_amd`` is imported from (default:
this tree), so the same file runs against another commit's package.  It hooks only what every build has:
  * the engine's library handle -- ``eng.lib`` is replaced, right after the engine is made and before any plan is built, by a proxy
    whose attributes call through; the steps of every plan then bind the proxy's callables;
  * ``torch.cuda.Event`` (creation, ``record``), ``torch.cuda.Stream.wait_event`` and ``torch.Tensor.record_stream``;
  * ``otvm_amd.lib.check`` (the label a direct call is checked under) and ``eng._frame_batch`` (where a frame call begins and ends).
Per frame call, in order: every library call as symbol | stream role (main / side / side2 / other, - for a call without a stream) |
label of the launch step it belongs to, or of its check -- and, for a call that is no step of a launch list (preprocess, crop, the
trimap kernels, the memory read, ...), its arguments, pointers as allocation + byte offset in plan_dump's naming (never an address);
every event record / wait as (number of the event in order of creation, stream role); every record_stream; then the bank's frame
ids, last_T_read and the growth of conv_calls.  Graphs are off, engine.AUTOTUNE is False, the launch stream is not the default one
(no stream handle is 0).  Synthetic weights; the cases are listed in CASES."""
import argparse
import ctypes as C
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))


def _plan_dump():
    """tools/plan_dump.py as a module (its allocation naming), wherever this file was imported from."""
    if "plan_dump" not in sys.modules:
        import importlib.util
        spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(HERE, "plan_dump.py"))
        sys.modules["plan_dump"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["plan_dump"])
    return sys.modules["plan_dump"]


class _Call:
    """One attribute of the library proxy: a callable that reports to the recorder and calls through.  A new one per attribute
    access, so that a launch step is recognised by the callable it bound."""
    __slots__ = ("fn", "__name__", "rec")

    def __init__(self, fn, name, rec):
        self.fn, self.__name__, self.rec = fn, name, rec

    def __call__(self, *args):
        if self.rec.active:
            self.rec.on_call(self, args)
        return self.fn(*args)


class _LibProxy:
    def __init__(self, lib, rec):
        self.__dict__["_lib"], self.__dict__["_rec"] = lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        return _Call(fn, name, self._rec) if name.startswith("otvm_") else fn


class Recorder:
    """``with Recorder(eng) as rec:`` -- while active, everything the engine ``eng`` issues is appended to ``rec.calls``: one dict
    per frame call (``depth`` 0, or deeper for a frame the conditioning guard computes again from inside the call) with its
    ``entries`` and, once it has returned, ``bank`` / ``T_read`` / ``conv_calls``; what is issued between frame calls (a flush) goes
    to a call of depth -1.  Entries: ("call", callable, args, stream role, check label), ("record" | "wait", event number, stream
    role), ("record_stream", tensor, stream role).  ``text()`` renders them.  The proxy stays on the engine (its steps are bound to
    it) and passes through once the recorder is closed."""

    def __init__(self, eng):
        import torch
        from otvm_amd import lib as L
        self.torch, self.L, self.eng = torch, L, eng
        self.active, self.calls, self.stack, self.events, self.slots, self.named = False, [], [], [], [], []
        self.main = None
        if not isinstance(eng.lib, _LibProxy):
            eng.lib = _LibProxy(eng.lib, self)
        else:
            eng.lib.__dict__["_rec"] = self

    # ---- hooks
    def __enter__(self):
        torch, L, eng, rec = self.torch, self.L, self.eng, self
        self.main = torch.cuda.current_stream(eng.dev).cuda_stream
        ev_cls, st_cls = torch.cuda.Event, torch.cuda.Stream
        self._saved = (ev_cls.__dict__["__new__"], ev_cls.record, st_cls.wait_event, torch.Tensor.record_stream, L.check)
        new0, record0, wait0, rs0, check0 = ev_cls.__new__, ev_cls.record, st_cls.wait_event, torch.Tensor.record_stream, L.check

        def new(cls, *a, **k):
            ev = new0(cls, *a, **k)
            rec.events.append(ev)                                 # (kept alive: the number of an event is its index)
            return ev

        def record(ev, stream=None):
            stream = torch.cuda.current_stream() if stream is None else stream
            rec.add(("record", rec.event_no(ev), rec.role(stream.cuda_stream)))
            return record0(ev, stream)

        def wait_event(stream, ev):
            rec.add(("wait", rec.event_no(ev), rec.role(stream.cuda_stream)))
            return wait0(stream, ev)

        def record_stream(t, stream):
            rec.add(("record_stream", t, rec.role(stream.cuda_stream)))
            return rs0(t, stream)

        def check(rc, what=""):
            cur = rec.current()["entries"] if rec.active else None
            if cur and cur[-1][0] == "call" and cur[-1][4] is None:
                cur[-1] = cur[-1][:4] + (what,)
            return check0(rc, what)

        frame_batch0 = eng._frame_batch

        def frame_batch(*a, **k):
            call = dict(depth=len(rec.stack), entries=[], conv0=eng.conv_calls, args=a[:4])
            rec.calls.append(call)
            rec.stack.append(call)
            try:
                call["ret"] = frame_batch0(*a, **k)
            finally:
                rec.stack.pop()
            call["bank"], call["T_read"], call["conv_calls"] = eng.bank_frames(), eng.last_T_read, eng.conv_calls - call["conv0"]
            call["text"] = rec.render(call)                       # now: while the plan and the tensors of this call are alive
            del call["args"]
            return call.pop("ret")

        ev_cls.__new__, ev_cls.record, st_cls.wait_event = staticmethod(new), record, wait_event
        torch.Tensor.record_stream, L.check, eng._frame_batch = record_stream, check, frame_batch
        self.active = True
        return self

    def __exit__(self, *exc):
        torch, L = self.torch, self.L
        self.active = False
        new0, record0, wait0, rs0, check0 = self._saved
        torch.cuda.Event.__new__, torch.cuda.Event.record, torch.cuda.Stream.wait_event = new0, record0, wait0
        del torch.Tensor.record_stream                            # (inherited from the base class again)
        L.check = check0
        del self.eng._frame_batch                                 # (the instance attribute: the method is back)

    # ---- recording
    def current(self):
        if self.stack:
            return self.stack[-1]
        if not self.calls or self.calls[-1]["depth"] != -1:
            self.calls.append(dict(depth=-1, entries=[]))
        return self.calls[-1]

    def add(self, entry):
        if self.active:
            self.current()["entries"].append(entry)

    def on_call(self, fn, args):
        keep = []
        for a in args:                                            # structures and arrays change under the engine's hands: copies
            obj = getattr(a, "_obj", None)
            if isinstance(obj, C.Structure):
                a = C.byref(type(obj).from_buffer_copy(obj))
            elif isinstance(a, C.Array):
                a = type(a)(*a)
            keep.append(a)
        types = self.L._PROTOS[fn.__name__][1]                    # a launch takes its stream last, as a void pointer
        role = self.role(args[-1]) if types and types[-1] is C.c_void_p and isinstance(args[-1], int) else None
        self.add(("call", fn, tuple(keep), None if role == "other" else role, None))   # (other: a pointer that is no stream of ours)

    def role(self, handle):
        eng = self.eng
        for name, s in (("side", eng.side), ("side2", eng.side2)):
            if s is not None and s.cuda_stream == handle:
                return name
        return "main" if handle == self.main else "other"

    def event_no(self, ev):
        for i, e in enumerate(self.events):
            if e is ev:
                return i
        self.events.append(ev)                                    # (made before the recorder was opened)
        return len(self.events) - 1

    # ---- facts the tests read
    def launches(self, call, key):
        """Stream roles of the launches of list ``key`` of the plan, in the order ``call`` issued them."""
        steps = {id(st.fn) for st in self.eng.last_plan.steps[key]}
        return [e[3] for e in call["entries"] if e[0] == "call" and id(e[1]) in steps]

    def symbols(self, call):
        """(position, symbol, stream role) of every library call and ("record" | "wait", event number, role) of every event."""
        return [(i,) + ((e[1].__name__, e[3]) if e[0] == "call" else e) for i, e in enumerate(call["entries"])
                if e[0] in ("call", "record", "wait")]

    # ---- text
    def _allocations(self, call):
        from otvm_amd.engine import Act
        eng, al = self.eng, _plan_dump().Allocations()
        for i, plan in enumerate(eng.plans.values()):
            for key, b in plan._bufs.items():
                al.add("plan%d.buf%s" % (i, key), b.t if isinstance(b, Act) else b)
            al.add("plan%d.stats" % i, plan.stats)
            al.add("plan%d.diag" % i, getattr(plan, "diag", None))
            for b, w in enumerate(plan.mem_ws or []):
                al.add("plan%d.mem_ws%d" % (i, b), w)
        pend = eng.pending
        pend = [] if pend is None else [pend["slot"] if isinstance(pend, dict) else pend.slot]
        for s in list(eng.bank) + list(eng.free_slots) + pend:
            if not any(s is k for k in self.slots):
                self.slots.append(s)
        for i, s in enumerate(self.slots):
            al.add("slot%d.k" % i, s["k"].t)
            al.add("slot%d.v" % i, s["v"].t)
            for b, p in enumerate(s.get("packed_b", [])):
                al.add("slot%d.packed%d" % (i, b), p)
        for name, cw in eng.W.items():
            for f in ("w", "w_hi", "w_lo", "w_scale", "w_frag", "w_wfrag", "w16", "bias"):
                al.add("W[%s].%s" % (name, f), getattr(cw, f, None))
        al.add("W_ppm", eng.W_ppm)
        for name, (mp, v) in eng.GP.items():
            al.add("GP[%s].Mp" % name, mp)
            al.add("GP[%s].v" % name, v)
        for name, t in eng.sd.items():
            al.add("sd[%s]" % name, t)
        al.add("guard_flag", eng.guard_flag)
        for what, lst in zip(("a", "fg", "bg", "tri_gt"), call.get("args", ())):
            for b, t in enumerate(lst):
                if self.torch.is_tensor(t) and t.is_cuda:
                    al.add("arg.%s%d" % (what, b), t)
        for b, out in enumerate(call.get("ret") or ()):
            for what, t in zip(("scaled_imgs", "tri_out", "tri_gt_out", "alpha"), out):
                al.add("ret%d.%s" % (b, what), t)
        for what in ("last_alpha_u8_b", "last_fgr_b", "last_rgba_u8_b", "last_comp_u8_b"):
            for b, t in enumerate(getattr(eng, what, None) or ()):
                al.add("%s%d" % (what, b), t)
        al.freeze()
        return al

    def _step_labels(self):
        eng, labels = self.eng, {}
        lists = [steps for plan in eng.plans.values() for steps in plan.steps.values()]
        lists += [s["kv_steps"] for s in self.slots if "kv_steps" in s]
        for steps in lists:
            for st in steps:
                labels.setdefault(id(st.fn), []).append(st)
        return labels

    def render(self, call):
        fmt_arg = _plan_dump().fmt_arg
        al, labels, out = self._allocations(call), self._step_labels(), []
        for e in call["entries"]:
            if e[0] != "call":
                what = al.name(e[1].data_ptr()) + " %s %s" % (e[1].dtype, tuple(e[1].shape)) if e[0] == "record_stream" else "event %d" % e[1]
                out.append("%s | %s | %s" % (e[0], what, e[2]))
                continue
            _, fn, args, role, checked = e
            largs = args[:-1] if role is not None else args
            step = next((st for st in labels.get(id(fn), ()) if st.args is not None and len(st.args) == len(largs)
                         and all(x is y or x == y for x, y in zip(st.args, largs) if not hasattr(x, "_obj") and not isinstance(x, C.Array))),
                        None)
            if step is not None:
                out.append("%s | %s | step %s" % (fn.__name__, role or "-", step.label))
                continue
            text = []
            for a, t in zip(largs, self.L._PROTOS[fn.__name__][1]):
                obj = getattr(a, "_obj", None)
                if obj is not None and not isinstance(obj, C.Structure):
                    text.append("&" + type(obj).__name__)         # (an output the library writes: its address says nothing)
                else:
                    text.append(fmt_arg(a, t, al))
            out.append("%s | %s | check %s | %s" % (fn.__name__, role or "-", checked, " ; ".join(text)))
        if "bank" in call:
            out.append("bank %r T_read %d conv_calls +%d" % (call["bank"], call["T_read"], call["conv_calls"]))
        return out

    def text(self):
        out = []
        for i, call in enumerate(self.calls):
            out.append("# call %d depth %d" % (i, call["depth"]))
            out += call["text"] if "text" in call else self.render(call)
        return out


# ------------------------------------------------------------------ the cases
H0, W0 = 64, 96            # pads to one plan; small maps, where the lock-step batch matters


def _clip(H, W, T, seed, planar=True, device=None):
    """(a, [fg per frame], tri_gt) as the model takes them: fp32 planar BGR host tensors, or uint8 [H,W,3] frames."""
    import numpy as np
    import torch
    from otvm_amd.synth_data import synthetic_clip
    frames, tri = synthetic_clip(H, W, T, seed=seed)
    if planar:
        fgs = [torch.from_numpy(frames[t].astype(np.float32)).permute(2, 0, 1)[None, None].contiguous() for t in range(T)]
    else:
        fgs = [torch.from_numpy(frames[t]).contiguous() for t in range(T)]
    a, tg = torch.ones(1, 1, 1, H, W), torch.from_numpy(tri)[None, None]
    if device is not None:
        a, tg, fgs = a.to(device), tg.to(device), [f.to(device) for f in fgs]
    return a, fgs, tg


def _run_clip(m, a, fgs, tg, every=2, max_num=3, last=True, **kw):
    T = len(fgs)
    for t in range(T):
        m(a, fgs[t], fgs[t].clone(), tri_gt=tg, first_frame=(t == 0), last_frame=(last and t == T - 1), memorize=(t % every == 0),
          max_memory_num=max_num, **kw)


def case_clip6(m, eng):
    _run_clip(m, *_clip(H0, W0, 6, 5))


def case_u8_ready(m, eng):
    _run_clip(m, *_clip(H0, W0, 4, 6, planar=False, device="cuda"), _inputs_ready=True, _frames_rgb=True)


def case_u8_event(m, eng):
    import torch
    a, fgs, tg = _clip(H0, W0, 4, 6, planar=False, device="cuda")
    for t in range(4):
        ev = torch.cuda.Event()
        ev.record()
        m(a, fgs[t], fgs[t].clone(), tri_gt=tg, first_frame=(t == 0), last_frame=(t == 3), memorize=(t % 2 == 0), max_memory_num=3,
          _inputs_ready=ev)


def case_no_side_stream(m, eng):
    eng.use_side_stream = False
    _run_clip(m, *_clip(H0, W0, 6, 5))


def case_f32(m, eng):
    _run_clip(m, *_clip(H0, W0, 4, 5))


def case_batch2(m, eng):
    a, f0, tg = _clip(H0, W0, 4, 5)
    _, f1, tg1 = _clip(H0, W0, 4, 7)
    for t in range(4):
        m.forward_batch([a, a], [f0[t], f1[t]], [f0[t].clone(), f1[t].clone()], [tg, tg1], first_frame=(t == 0), last_frame=(t == 3),
                        memorize=(t % 2 == 0), max_memory_num=3)


def case_trimap_from_alpha(m, eng):
    import torch
    a, fgs, tg = _clip(H0, W0, 3, 5)
    a = tg[:, :, 2:3].clone() + 0.5 * tg[:, :, 1:2]               # an alpha with all three regions
    for t in range(3):
        m(a, fgs[t], fgs[t].clone(), tri_gt=None, first_frame=(t == 0), last_frame=(t == 2), memorize=True, max_memory_num=3)
    torch.cuda.synchronize()


def case_keyframe_labels(m, eng):
    import torch
    a, fgs, tg = _clip(H0, W0, 5, 5)
    lab = tg[0, 0].argmax(0).to(torch.uint8)
    lab[: H0 // 2] = 255                                          # the upper half is unlabelled
    for t in range(5):
        kw = dict(tri_gt=tg, keyframe=True) if t == 2 else dict(tri_gt=tg, keyframe=True, labels=lab) if t == 3 else dict(tri_gt=tg)
        m(a, fgs[t], fgs[t].clone(), first_frame=(t == 0), last_frame=(t == 4), memorize=(t % 2 == 0), max_memory_num=3, **kw)


def case_foreground(m, eng):
    m.foreground = True
    m.set_background((0, 255, 0))
    _run_clip(m, *_clip(H0, W0, 3, 5, planar=False, device="cuda"))
    m.foreground = False
    m.set_background(None)


def case_train(m, eng):
    import numpy as np
    import torch
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.train import train_forward
    frames, tri = synthetic_clip(H0, W0, 3, seed=5)
    fg = torch.from_numpy(frames.astype(np.float32)).permute(0, 3, 1, 2)[None].contiguous()
    tri = torch.from_numpy(tri)[None, None].repeat(1, 3, 1, 1, 1).contiguous()
    train_forward(m, tri[:, :, 2:3].contiguous(), fg, fg.flip(-1).contiguous(), tri)


def case_prof(m, eng):
    eng.prof = []
    _run_clip(m, *_clip(H0, W0, 3, 5))


def case_check_level3(m, eng):
    eng.check_level = 3
    _run_clip(m, *_clip(H0, W0, 3, 5))


def case_dropped_pending(m, eng):
    clip = _clip(H0, W0, 3, 5)
    _run_clip(m, *clip, last=False)                               # ends without last_frame: its memorize stays pending ...
    _run_clip(m, *clip)                                           # ... and is dropped by the next first frame


def case_resolution_change(m, eng):
    a, fgs, tg = _clip(H0, W0, 2, 5)
    _run_clip(m, a, fgs, tg, last=False)
    a2, f2, tg2 = _clip(70, 90, 1, 5)                             # another plan, the memorize of frame 1 pending: a full keyframe (no
    m(a2, f2[0], f2[0].clone(), tri_gt=tg2, keyframe=True, last_frame=True, max_memory_num=3)   # read of the other plan's slots)


def case_pre_on_main(m, eng):
    _run_clip(m, *_clip(H0, W0, 4, 5))


def case_evdec_early(m, eng):
    _run_clip(m, *_clip(H0, W0, 4, 5))


def case_guard_p3(m, eng):
    _run_clip(m, *_clip(H0, W0, 2, 31))


def case_guard_off(m, eng):
    _run_clip(m, *_clip(H0, W0, 2, 31))
    _run_clip(m, *_clip(H0, W0, 2, 31))                           # the next clip: plans without the predicted tails


# name -> (case, model precision, {engine module global: value while the case runs})
GUARD = dict(GN_PREDICT_MIN_PIXELS=0)
CASES = {
    "clip6": (case_clip6, None, {}), "u8_ready": (case_u8_ready, None, {}), "u8_event": (case_u8_event, None, {}),
    "no_side_stream": (case_no_side_stream, None, {}), "f32": (case_f32, "f32", {}), "batch2": (case_batch2, None, {}),
    "trimap_from_alpha": (case_trimap_from_alpha, None, {}), "keyframe_labels": (case_keyframe_labels, None, {}),
    "foreground": (case_foreground, None, {}), "train": (case_train, None, {}), "prof": (case_prof, None, {}),
    "check_level3": (case_check_level3, None, {}), "dropped_pending": (case_dropped_pending, None, {}),
    "resolution_change": (case_resolution_change, None, {}), "pre_on_main": (case_pre_on_main, None, dict(PRE_ON_S2=False)),
    "evdec_early": (case_evdec_early, None, dict(EVDEC_LATE=False)),
    "guard_p3": (case_guard_p3, None, dict(GUARD, GN_PREDICT_KAPPA_P3=-1.0, GN_PREDICT_KAPPA_OFF=1e30)),
    "guard_off": (case_guard_off, None, dict(GUARD, GN_PREDICT_KAPPA_OFF=-1.0)),
}


def make_model():
    from otvm_amd import helpers
    from otvm_amd.synth_weights import synthetic_state_dict
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
    m.load_state_dict(synthetic_state_dict(0), strict=True)
    return m.cuda().eval()


def run_case(m, name):
    """The text of case ``name``: a new engine for the model ``m``, its library handle replaced before any plan exists."""
    import torch
    from otvm_amd import engine
    case, precision, patch = CASES[name]
    saved = {k: getattr(engine, k) for k in patch}
    for k, v in patch.items():
        setattr(engine, k, v)
    try:
        m.precision, m._engine = precision, None
        eng = m._get_engine()
        eng.use_graphs = False
        with torch.cuda.stream(torch.cuda.Stream()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with Recorder(eng) as rec:
                case(m, eng)
                eng.flush()
            torch.cuda.synchronize()
        return ["## case %s" % name] + rec.text()
    finally:
        for k, v in saved.items():
            setattr(engine, k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the directory otvm_amd is imported from")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out")
    args = ap.parse_args()
    os.environ["OTVM_GRAPHS"] = "0"
    sys.path.insert(0, os.path.abspath(args.root))
    from otvm_amd import engine
    engine.AUTOTUNE = False
    m, out = make_model(), []
    for name in args.cases.split(","):
        out += run_case(m, name)
        print("case %s: %d lines so far" % (name, len(out)), file=sys.stderr, flush=True)
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
