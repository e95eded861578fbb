"""CPU: the plan-time tuner of otvm_amd/engine.py -- the one timing protocol (_time_candidates), the one decision ladder
(_choose) and the two call sites that can be driven without a device (FramePlan.tune_convs, FramePlan._resolve_stm128).  A fake
clock and recording launch functions stand in for the device and the library; nothing here opens a GPU or loads the library."""
import ctypes
from types import SimpleNamespace

import pytest

from otvm_amd import engine
from otvm_amd import lib as L


class FakeClock:
    """mark() writes "|" into the launch record (so a test sees where the timed span begins and ends); ms() hands out the
    scripted times, given per repetition, and counts how often the device was waited for."""
    stream = 0

    def __init__(self, log, per_rep, reps=3):
        self.log, self.per_rep, self.reps, self.waits = log, list(per_rep), reps, 0

    def mark(self):
        self.log.append("|")
        return len(self.log)

    def ms(self, pairs):
        self.waits += 1
        assert all(b > a for a, b in pairs)
        out, self.per_rep = self.per_rep[:len(pairs)], self.per_rep[len(pairs):]
        assert len(out) == len(pairs)
        return [t * self.reps for t in out]


def recorder(log, what):
    def launch(*args):
        assert args[-1] == FakeClock.stream                     # the stream comes last, as in every library call
        log.append(what() if callable(what) else what)
        return 0
    return launch


def rt(ms):
    """The scripted per-repetition times after their round trip through the clock (x reps, / reps)."""
    return {c: t * 3 / 3 for c, t in ms.items()}


def measurement(c, lead=0, reps=3, per_rep=1):
    return [c] * (lead * per_rep) + ["|"] + [c] * (reps * per_rep) + ["|"]


@pytest.fixture
def tune_state(monkeypatch):
    """An empty cache and log of this test's own, and no tune file."""
    monkeypatch.setattr(engine, "_TUNE_CACHE", {})
    monkeypatch.setattr(engine, "TUNE_LOG", [])
    monkeypatch.setattr(engine, "TUNE_FILE", None)
    return engine


def test_conv_protocol_launch_sequence_and_minimum():
    """Conv shape with the candidates [0, 35, 51]: 3 launches of code 0 thrown away, then for each of 0, 35, 51, 0 one untimed
    launch and three timed ones -- 3 + 4 * 4 = 19 conv launches; the incumbent's time is the smaller of its two measurements."""
    log, code = [], [None]
    step = engine.Step(recorder(log, lambda: code[0]), ("params",), "conv layer", True)

    def steps_of(c):
        code[0] = c
        return (step,)
    eng = SimpleNamespace(conv_calls=5)
    clock = FakeClock(log, [2.0, 1.5, 3.0, 1.0])
    ms = engine._time_candidates(eng, clock, steps_of, [0, 35, 51] + [0], 3, warm=(0, 0, 0), lead=1)
    assert log == [0, 0, 0] + measurement(0, 1) + measurement(35, 1) + measurement(51, 1) + measurement(0, 1)
    assert eng.conv_calls - 5 == 19 == 3 + 4 * (3 + 1)
    assert clock.waits == 1
    assert ms == rt({0: 1.0, 35: 1.5, 51: 3.0})                      # 0: the minimum (the LAST of its measurements here)


def test_stm128_protocol_launch_sequence_and_minimum():
    """Planes-128 block: 2 untimed repetitions of route 0 (three launches each), then 0,1,2,3,0,1,2,3 at 3 repetitions with
    nothing in between -- 42 conv launches; the result is the minimum, neither the last measurement nor the mean."""
    log = []
    U = [engine.Step(recorder(log, "u%d" % i), (), "conv block.conv%d" % i, True) for i in (1, 2, 3)]
    fused = engine.Step(recorder(log, "f"), (), "conv block (fused bottleneck)", True)
    eng = SimpleNamespace(conv_calls=0)
    clock = FakeClock(log, [1.0, 5.0, 3.0, 4.0, 2.0, 4.0, 6.0, 4.5])
    ms = engine._time_candidates(eng, clock, lambda c: U if c == 0 else (fused,), (0, 1, 2, 3, 0, 1, 2, 3), 3, warm=(0, 0))
    u = ["u1", "u2", "u3"]
    one_round = ["|"] + u * 3 + ["|"] + (["|"] + ["f"] * 3 + ["|"]) * 3
    assert log == u * 2 + one_round * 2
    assert eng.conv_calls == 42 and clock.waits == 1
    assert ms == rt({0: 1.0, 1: 4.0, 2: 3.0, 3: 4.0})             # 0: its FIRST measurement, 1: its last, 2: not the mean 4.5


@pytest.mark.parametrize("readers", [1, 2])
def test_upfold_protocol_launch_sequence(readers):
    """Folded upsampling: 2 untimed repetitions of each route, then 0,1,0,1,0,1,0,1 at 3 repetitions -- 28 conv launches per
    reader (the upsampling pass of route 0 is launched with them and is not a conv)."""
    log = []
    r0 = [engine.Step(recorder(log, "up"), (), "upsample")]
    r0 += [engine.Step(recorder(log, "r%d" % i), (), "conv reader%d" % i, True) for i in range(readers)]
    r1 = [engine.Step(recorder(log, "R%d" % i), (), "conv reader%d (+ up2x)" % i, True) for i in range(readers)]
    routes = {0: r0, 1: r1}
    eng = SimpleNamespace(conv_calls=0)
    clock = FakeClock(log, [3.0, 2.0, 2.5, 2.2, 2.9, 1.9, 2.6, 2.1])
    ms = engine._time_candidates(eng, clock, routes.get, (0, 1) * 4, 3, warm=(0, 0, 1, 1))
    a = ["up"] + ["r%d" % i for i in range(readers)]
    b = ["R%d" % i for i in range(readers)]
    assert log == a * 2 + b * 2 + (["|"] + a * 3 + ["|"] + ["|"] + b * 3 + ["|"]) * 4
    assert eng.conv_calls == 28 * readers and clock.waits == 1
    assert ms == rt({0: 2.5, 1: 1.9})


def test_every_launch_is_checked(monkeypatch):
    """Every launch's return code goes through L.check: an error stops the timing, whichever launch of whichever candidate
    it is.  (L.check itself asks the library for the error text: replaced here, no library on this path.)"""
    log, checked = [], []

    def check(rc, what=""):
        checked.append(what)
        if rc != 0:
            raise RuntimeError(what)
    monkeypatch.setattr(L, "check", check)
    bad = engine.Step(lambda *a: 7, (), "conv broken", True)
    good = engine.Step(recorder(log, "g"), (), "conv fine", True)
    eng = SimpleNamespace(conv_calls=0)
    with pytest.raises(RuntimeError):
        engine._time_candidates(eng, FakeClock(log, [1.0, 1.0]), lambda c: (good, bad) if c else (good,), (0, 1), 3, warm=(0,))
    assert log == ["g", "|", "g", "g", "g", "|", "|", "g"]        # stopped at route 1's second launch of its first repetition
    assert checked == ["conv fine"] * 5 + ["conv broken"]


@pytest.mark.parametrize("default", [-1, 0])                      # the planes-128 block's and the upfold's untimed default
def test_decision_ladder(tune_state, default):
    calls = []

    def measure():
        calls.append(1)
        return {0: 2.0, 1: 1.999, 2: 2.5}
    key, sig = (-128, 6, 8, 1, 512, 512), (6, 8, 512, 512, 512, 512, 3, 3, 1, 1, 1)
    engine._TUNE_CACHE[key] = 2
    # forced wins over the cache; nothing is timed
    assert engine._choose(key, "label", sig, measure, forced=3, default=None) == 3
    # cached wins over timing and over the default
    assert engine._choose(key, "label", sig, measure, forced=None, default=None) == 2
    assert engine._choose(key, "label", sig, measure, forced=None, default=default) == 2
    assert calls == [] and engine.TUNE_LOG == [] and engine._TUNE_CACHE == {key: 2}
    # timing off, nothing cached: the default, NOT stored
    engine._TUNE_CACHE.clear()
    assert engine._choose(key, "label", sig, measure, forced=None, default=default) == default
    assert calls == [] and engine._TUNE_CACHE == {} and engine.TUNE_LOG == []
    # timed: no margin -- the smaller time wins however close; stored under the key, logged once
    assert engine._choose(key, "label", sig, measure, forced=None, default=None) == 1
    assert calls == [1] and engine._TUNE_CACHE == {key: 1}
    assert engine.TUNE_LOG == [("label", sig, 1, {0: 2.0, 1: 1.999, 2: 2.5})]
    # ... and not timed again
    assert engine._choose(key, "label", sig, measure, forced=None, default=None) == 1
    assert calls == [1] and len(engine.TUNE_LOG) == 1


class FakeConvLib:
    """otvm_conv2d_candidates offers ``codes``; otvm_conv2d records the tune code it was launched with."""

    def __init__(self, log, codes):
        self.log, self.codes = log, codes

    def otvm_conv2d_candidates(self, ref, out, n):
        for i, c in enumerate(self.codes):
            out[i] = c
        return len(self.codes)

    def otvm_conv2d(self, ref, stream):
        self.log.append(int(ref._obj.tune))
        return 0


def fake_plan(lib):
    plan = object.__new__(engine.FramePlan)
    plan.e = SimpleNamespace(precision=L.PREC_F16X3, conv_calls=0)
    plan.lib, plan.dev = lib, None
    return plan


@pytest.mark.parametrize("ratio, chosen", [(0.98, 0), (0.96, 35)])
def test_conv_call_site(tune_state, monkeypatch, ratio, chosen):
    """FramePlan.tune_convs on a fake library: the launch sequence of the protocol, the one-wave tile (codes 160 .. 175) left
    out while WAVE_TILE is off, and the 3 % rule -- a code at 0.98 x the incumbent's time loses to code 0, one at 0.96 x wins."""
    log = []
    clock = FakeClock(log, [1.1, ratio, 2.0, 1.0])               # measurements of 0, 35, 51, 0: the incumbent's best is 1.0
    monkeypatch.setattr(engine, "_EventClock", lambda dev: clock)
    monkeypatch.setattr(engine, "AUTOTUNE", True)
    monkeypatch.setattr(engine, "WAVE_TILE", False)
    plan = fake_plan(FakeConvLib(log, [35, 165, 51]))
    p, twin = L.ConvParams(), L.ConvParams()
    p.H = twin.H = 6
    p.tune = twin.tune = 99
    plan.tune_convs([(p, "layer"), (twin, "twin of layer")])
    assert log == [0, 0, 0] + measurement(0, 1) + measurement(35, 1) + measurement(51, 1) + measurement(0, 1)
    assert plan.e.conv_calls == 19                               # the twin has the same signature: a cache hit, not timed
    assert p.tune == twin.tune == chosen
    sig = engine.FramePlan._signature(p)
    assert engine._TUNE_CACHE == {sig: chosen}
    assert engine.TUNE_LOG == [("layer", sig, chosen, rt({0: 1.0, 35: ratio, 51: 2.0}))]


def test_timed_choices_are_saved_once_per_phase(tune_state, monkeypatch):
    """Two signatures timed in one tune_convs phase: ONE write of the tune file, after both; a phase of cache hits writes nothing."""
    log, saves = [], []
    clock = FakeClock(log, [1.0, 2.0, 1.0] * 2)
    monkeypatch.setattr(engine, "_EventClock", lambda dev: clock)
    monkeypatch.setattr(engine, "_save_tune_file", lambda: saves.append(dict(engine._TUNE_CACHE)))
    monkeypatch.setattr(engine, "AUTOTUNE", True)
    plan = fake_plan(FakeConvLib(log, [35]))
    p, q = L.ConvParams(), L.ConvParams()
    p.H, q.H = 6, 12
    plan.tune_convs([(p, "a"), (q, "b")])
    sp, sq = engine.FramePlan._signature(p), engine.FramePlan._signature(q)
    assert saves == [{sp: 0, sq: 0}]
    plan.tune_convs([(p, "a"), (q, "b")])
    assert len(saves) == 1 and len(engine.TUNE_LOG) == 2


def stm128_plan(log, monkeypatch, per_rep):
    clock = FakeClock(log, per_rep)
    monkeypatch.setattr(engine, "_EventClock", lambda dev: clock)
    q = L.StmBottleneckParams()
    q.H, q.W, q.batch, q.x_ld, q.y_ld = 12, 16, 1, 512, 512
    U = [engine.Step(recorder(log, "u%d" % i), (), "conv res3.1.conv%d" % i, True) for i in (1, 2, 3)]
    fused = engine.Step(recorder(log, lambda: "f%d" % q.tile), (ctypes.byref(q),), "conv res3.1 (fused bottleneck)", True)
    before, after = engine.Step("before", (), "maxpool"), engine.Step("after", (), "conv next", True)
    S = [before, fused, after]
    plan = fake_plan(None)
    plan._stm128 = [(S, fused, U, q, "res3.1")]
    return plan, S, U, fused, q, before, after


def test_stm128_call_site_timed(tune_state, monkeypatch):
    """FramePlan._resolve_stm128, timing on: routes 0,1,2,3 twice, 42 conv launches, no margin (3.99 beats 4.0), and the
    placeholder replaced by the chosen route."""
    log = []
    plan, S, U, fused, q, before, after = stm128_plan(log, monkeypatch, [4.0, 5.0, 6.0, 7.0, 4.1, 5.0, 3.99, 7.0])
    monkeypatch.setattr(engine, "FUSE_STM_BLOCK128", 1)
    plan._resolve_stm128(timed=True)
    u = ["u1", "u2", "u3"]
    one_round = ["|"] + u * 3 + ["|"] + ["|"] + ["f1"] * 3 + ["|"] + ["|"] + ["f2"] * 3 + ["|"] + ["|"] + ["f3"] * 3 + ["|"]
    assert log == u * 2 + one_round * 2
    assert plan.e.conv_calls == 42
    key = (-128, 12, 16, 1, 512, 512)
    assert engine._TUNE_CACHE == {key: 2} and q.tile == 2 and S == [before, fused, after] and plan._stm128 == []
    (name, sig, choice, ms), = engine.TUNE_LOG
    assert name.startswith("res3.1 (fused bottleneck") and sig == (12, 16, 512, 512, 512, 512, 3, 3, 1, 1, 1)
    assert choice == 2 and ms == rt({0: 4.0, 1: 5.0, 2: 3.99, 3: 7.0})


@pytest.mark.parametrize("switch, tile, timed, cached, expect", [
    (2, 0, True, 0, -1),        # forced "always": the library picks the tile, whatever the cache says
    (2, 3, True, 0, 3),         # forced tile
    (1, 0, True, 0, 0),         # cached: the three launches
    (1, 0, False, 1, 1),        # cached, no tuner
    (1, 0, False, None, -1),    # nothing cached, no tuner: fused, the library picks
])
def test_stm128_call_site_untimed(tune_state, monkeypatch, switch, tile, timed, cached, expect):
    log = []
    plan, S, U, fused, q, before, after = stm128_plan(log, monkeypatch, [])
    monkeypatch.setattr(engine, "FUSE_STM_BLOCK128", switch)
    monkeypatch.setattr(engine, "STM128_TILE", tile)
    key = (-128, 12, 16, 1, 512, 512)
    if cached is not None:
        engine._TUNE_CACHE[key] = cached
    cache0 = dict(engine._TUNE_CACHE)
    plan._resolve_stm128(timed=timed)
    assert log == [] and plan.e.conv_calls == 0 and engine.TUNE_LOG == [] and engine._TUNE_CACHE == cache0
    if expect == 0:
        assert S == [before] + U + [after]
    else:
        assert S == [before, fused, after] and q.tile == max(expect, 0)
