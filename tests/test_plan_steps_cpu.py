"""CPU: the launch steps of otvm_amd/engine.py -- the one record (Step), the one loop that launches them (_issue) in its three modes,
the late arguments of the steps that need the GroupNorm statistics arena (FramePlan.late_step / _bind_stats) and the helper the
plan-time route choices splice with (_splice).  Recording functions stand in for the library, the engine's guard and HIP events;
nothing here opens a GPU or loads the library."""
from types import SimpleNamespace

import pytest
import torch

from otvm_amd import engine
from otvm_amd import lib as L
from otvm_amd.engine import Act, Step

STREAM = 77
MODES = ["plain", "prof", "level3"]


def recorder(log, what, rc=0):
    def launch(*args):
        assert args[-1] == STREAM                                # the stream comes last, as in every library call
        log.append((what,) + args[:-1])
        return rc
    return launch


class FakeEngine:
    """guard / scan_now as the executor calls them: recorded with the view and the text."""

    def __init__(self, log):
        self.log = log

    def guard(self, act, what, stream):
        assert stream == STREAM
        self.log.append(("guard", act, what))

    def scan_now(self, act, what, stream):
        assert stream == STREAM
        self.log.append(("scan", act, what))


@pytest.fixture
def events(monkeypatch):
    """torch.cuda.Event replaced: record() writes ("event", n-th event made) into the log handed back."""
    log = []

    class Event:
        made = 0

        def __init__(self, enable_timing=False):
            assert enable_timing
            Event.made += 1
            self.n = Event.made

        def record(self):
            log.append(("event", self.n))
    monkeypatch.setattr(engine.torch.cuda, "Event", Event)
    return log


@pytest.fixture
def checked(monkeypatch):
    """L.check replaced (the real one asks the library for the error text): notes what it was handed, raises on an error."""
    seen = []

    def check(rc, what=""):
        seen.append((rc, what))
        if rc != 0:
            raise RuntimeError(what)
    monkeypatch.setattr(L, "check", check)
    return seen


def issue(mode, steps, log, prof):
    """The three callers' argument forms: FramePlan.run's direct launch, its instrumented pass, its pass at check level 3."""
    if mode == "plain":
        engine._issue(steps, STREAM)
    elif mode == "prof":
        engine._issue(steps, STREAM, FakeEngine(log), prof, scan=False, guard_in=False)
    else:
        engine._issue(steps, STREAM, FakeEngine(log), None, scan=True, guard_in=True)


def three_steps(log, rc=(0, 0, 0)):
    src, dst = object(), object()
    return [Step(recorder(log, "pool", rc[0]), (1, 2), "maxpool"),
            Step(recorder(log, "conv", rc[1]), ("p",), "conv layer", True, 1000, 40, src, dst),
            Step(recorder(log, "gn", rc[2]), ("q",), "gn_apply layer")], src, dst


def test_executor_call_order_plain(events, checked):
    log = events
    steps, _, _ = three_steps(log)
    issue("plain", steps, log, None)
    assert log == [("pool", 1, 2), ("conv", "p"), ("gn", "q")]
    assert checked == []                                         # the direct launch hands L.check errors only


def test_executor_call_order_prof(events, checked):
    """Instrumented pass: two events around the convolution alone, its entry the 5-tuple bench.py reads."""
    log, prof = events, []
    steps, _, _ = three_steps(log)
    issue("prof", steps, log, prof)
    assert log == [("pool", 1, 2), ("event", 1), ("conv", "p"), ("event", 2), ("gn", "q")]
    (label, flops, e0, e1, abytes), = prof
    assert (label, flops, abytes, e0.n, e1.n) == ("conv layer", 1000, 40, 1, 2)
    # ... and with the check level at 3 as well (FramePlan.run, kv_into_slot): the timing alone, nothing scanned
    del log[:], prof[:]
    engine._issue(steps, STREAM, FakeEngine(log), prof, scan=True, guard_in=True)
    assert [e[0] for e in log] == ["pool", "event", "conv", "event", "gn"] and len(prof) == 1


def test_executor_call_order_level3(events, checked):
    """Check level 3: the convolution's input guarded in front of it, its output scanned behind it; kv_into_slot's form scans only."""
    log = events
    steps, src, dst = three_steps(log)
    issue("level3", steps, log, None)
    assert log == [("pool", 1, 2), ("guard", src, "input of conv layer"), ("conv", "p"), ("scan", dst, "output of conv layer"),
                   ("gn", "q")]
    del log[:]
    engine._issue(steps, STREAM, FakeEngine(log), None, scan=True)
    assert log == [("pool", 1, 2), ("conv", "p"), ("scan", dst, "output of conv layer"), ("gn", "q")]
    # check level below 3, no profile (kv_into_slot, the tuner): launches only, every return code through L.check
    del log[:], checked[:]
    engine._issue(steps, STREAM, FakeEngine(log), None, scan=False)
    assert log == [("pool", 1, 2), ("conv", "p"), ("gn", "q")]
    assert checked == [(0, "maxpool"), (0, "conv layer"), (0, "gn_apply layer")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bad", [0, 1])
def test_error_code_stops_the_sequence(events, checked, mode, bad):
    log, prof = events, []
    rc = [0, 0, 0]
    rc[bad] = 7
    steps, src, dst = three_steps(log, rc)
    with pytest.raises(RuntimeError, match=steps[bad].label):
        issue(mode, steps, log, prof)
    assert checked[-1] == (7, steps[bad].label)
    launched = [e[0] for e in log if e[0] in ("pool", "conv", "gn")]
    assert launched == ["pool", "conv"][:bad + 1]
    assert prof == [] and not any(e[0] == "scan" for e in log)    # a failed convolution is neither profiled nor scanned


@pytest.mark.parametrize("mode", MODES)
def test_unbound_late_arguments_are_refused(events, checked, mode):
    log = events
    steps, _, _ = three_steps(log)
    steps[1] = Step(recorder(log, "conv"), None, "conv late", True, 1, 1, object(), object(), late=lambda base, sbs: (base, sbs))
    with pytest.raises(RuntimeError, match="conv late"):
        issue(mode, steps, log, [])
    assert log == [("pool", 1, 2)]                               # nothing of the unbound step, nothing behind it
    plan = object.__new__(engine.FramePlan)
    plan.stats, plan.stats_bs = SimpleNamespace(data_ptr=lambda: 0x1000), 192
    plan._fused_stats, plan._late = [], [steps[1]]
    plan._bind_stats()
    assert steps[1].args == (0x1000, 192) and steps[1].late is None and plan._late == []
    del log[:]
    issue("plain", steps, log, None)
    assert log == [("pool", 1, 2), ("conv", 0x1000, 192), ("gn", "q")]


def test_late_arguments_after_binding():
    """The four kinds of step that need the statistics arena, on a plan with three GroupNorms, two images and the arena at 0x1000:
    block idx lies at base + idx * 512, an image's statistics stats_bs = 3 * 64 doubles behind the previous image's."""
    log = []
    names = ("otvm_gn_stats_b", "otvm_gn_table_b", "otvm_gn_apply_b", "otvm_ppm_conv_add")
    plan = object.__new__(engine.FramePlan)
    plan.lib = SimpleNamespace(**{n: recorder(log, n) for n in names})
    plan.dev, plan.B, plan.n_gn = torch.device("cpu"), 2, 0
    plan._bufs, plan._keep, plan._fused_stats, plan._late = {}, [], [], []
    sd = {"%s.%s" % (g, k): torch.zeros(8) for g in ("gn_a", "gn_b", "gn_c") for k in ("weight", "bias")}
    plan.e = SimpleNamespace(sd=sd)
    x = Act(torch.zeros(2 * 6 * 8), 2, 3, 8, B=2, bs=48)
    u1 = Act(torch.zeros(2 * 6 * 8), 2, 3, 8, B=2, bs=48)
    plan.PPM_Z = [torch.zeros(4), torch.zeros(4)]
    producer = SimpleNamespace(gn_stats=0, gn_bs=0)              # (not an otvm_conv_params: the table takes a launch of its own)
    S = []
    plan.gn(S, x, "gn_a", engine.RELU)                           # block 0: statistics pass + apply
    sc, sh, nbs = plan.gn_table_step(S, x, "gn_b", producer)     # block 1: statistics from the producer, table launch
    plan.ppm_conv_add(S, u1)                                     # block 2: summed by the gather, one launch per image
    plan.gn(S, u1, "gn_c", engine.LEAKY, stats_summed=True)
    assert plan.n_gn == 3 and [st.label for st in S] == ["gn_stats gn_a", "gn_apply gn_a", "gn_table gn_b", "ppm_conv_add",
                                                         "ppm_conv_add", "gn_apply gn_c"]
    assert all(st.args is None and not st.conv for st in S) and plan._late == S
    assert [st.fn for st in S] == [getattr(plan.lib, n) for n in (names[0], names[2], names[1], names[3], names[3], names[2])]
    plan.stats = SimpleNamespace(data_ptr=lambda: 0x1000)
    plan.stats_bs = max(plan.n_gn, 1) * 64
    plan._bind_stats()
    assert plan._late == [] and all(st.late is None for st in S)
    assert (producer.gn_stats, producer.gn_bs) == (0x1000 + 512, 192)
    engine._issue(S, STREAM)
    tab = plan._bufs[("raw", "gntab_gn_b", 2 * 8 * 2, torch.float32)].data_ptr()
    assert (sc, sh, nbs) == (tab, tab + 32, 16)
    stats, apply_a, table, add0, add1, apply_c = log
    assert stats == ("otvm_gn_stats_b", x.ptr, 6, 8, 8, 0x1000, 2, 48, 192)
    assert table == ("otvm_gn_table_b", 0x1000 + 512, 6, 8, sd["gn_b.weight"].data_ptr(), sd["gn_b.bias"].data_ptr(), tab, tab + 32,
                     2, 192, 16)
    assert add0 == ("otvm_ppm_conv_add", plan.PPM_Z[0].data_ptr(), 2, 3, u1.img(0).ptr, 8, 0x1000 + 1024)
    assert add1 == ("otvm_ppm_conv_add", plan.PPM_Z[1].data_ptr(), 2, 3, u1.img(1).ptr, 8, 0x1000 + 1024 + 8 * 192)
    for (name, ref), block, gamma in ((apply_a, 0, "gn_a"), (apply_c, 2, "gn_c")):
        q = ref._obj
        assert name == "otvm_gn_apply_b" and (q.stats, q.stats_bs) == (0x1000 + 512 * block, 192)
        assert (q.gamma, q.batch, q.x_bs) == (sd[gamma + ".weight"].data_ptr(), 2, 48)


class Same:
    """Steps that all compare equal as values: only identity tells them apart."""

    def __init__(self, label):
        self.label = label

    def __eq__(self, other):
        return isinstance(other, Same)
    __hash__ = None


@pytest.mark.parametrize("n_new", [0, 1, 3])
def test_splice_replaces_by_identity(n_new):
    a, b, c = Same("a"), Same("b"), Same("c")
    new = [Same("n%d" % i) for i in range(n_new)]
    S = [a, b, c]
    assert S.index(b) == 0                                       # (a search by value finds the wrong one)
    engine._splice(S, b, new)
    assert [st.label for st in S] == ["a"] + [st.label for st in new] + ["c"]
    assert all(x is y for x, y in zip(S, [a] + new + [c]))


def test_splice_raises_when_the_step_is_missing():
    S = [Same("a"), Same("b")]
    with pytest.raises(ValueError, match="'z'"):
        engine._splice(S, Same("z"), [])
    assert [st.label for st in S] == ["a", "b"]
