"""The host-only pieces of the engine's frame step (otvm_amd/engine.py): the argument refusals, the record of the deferred memorize
with its bank policy, the split of the early memory read, and the conditioning guard's retry decision.  No device."""
import itertools

import pytest

from otvm_amd.engine import (DROP_RECOMPUTE, GO_ON, RECOMPUTE, WARN_SUSPECT, Pending, bank_update, early_read_split,
                             refuse_frame_args, retry_decision)


def _refuse(n=1, tri_gt=True, first_frame=False, keyframe=False, labels=None, max_memory_num=3, train=None):
    tri = ["tri"] if tri_gt else [None]
    return refuse_frame_args(["a"] * n, ["fg"] * n, ["bg"] * n, tri * n, first_frame, keyframe, labels, max_memory_num, train)


def test_refusals_are_the_frame_steps():
    """The calls tests/test_gpu_keyframes.py::test_frame_step_refusals makes, with the engine's message texts."""
    lab = object()
    with pytest.raises(ValueError, match="labels correct a propagated trimap; a first frame takes its trimap as tri_gt"):
        _refuse(first_frame=True, labels=lab)
    with pytest.raises(ValueError, match="keyframe=True needs the frame's trimap as tri_gt"):
        _refuse(tri_gt=False, keyframe=True)
    with pytest.raises(ValueError, match=r"keyframe / labels need max_memory_num >= 2 \(a bank of 1 slot\(s\) holds no anchors\)"):
        _refuse(keyframe=True, max_memory_num=1)
    with pytest.raises(ValueError, match=r"keyframe / labels need max_memory_num >= 2 \(a bank of 0 slot\(s\) holds no anchors\)"):
        _refuse(labels=lab, max_memory_num=0)
    for kw in (dict(n=2, keyframe=True), dict(n=2, labels=lab), dict(keyframe=True, train={}), dict(labels=lab, train={})):
        with pytest.raises(NotImplementedError, match=r"keyframe / labels apply to a single sequence \(not to lock-step batches\)"):
            _refuse(**kw)
    with pytest.raises(ValueError, match="a / fg / bg / tri_gt lists must have the same length"):
        refuse_frame_args(["a"], ["fg"], ["bg", "bg"], ["tri"], False, False, None, 3, None)
    with pytest.raises(ValueError, match="a / fg / bg / tri_gt lists must have the same length"):
        refuse_frame_args([], [], [], [], False, False, None, 3, None)
    # what the same test runs without a refusal: first frame, last frame, and the options where they apply
    for kw in (dict(first_frame=True), dict(), dict(keyframe=True), dict(labels=lab), dict(labels=lab, keyframe=True, tri_gt=False),
               dict(n=2), dict(n=2, train={}), dict(max_memory_num=0), dict(first_frame=True, keyframe=True)):
        assert _refuse(**kw) is None


def _schedules():
    """(max_memory_num, [(first_frame, memorize, anchor) per frame]): the schedules of test_bank_policy_engine_equals_oracle, and the
    same with keyframes (anchors) spread over the clip."""
    for max_num in (0, 1, 2, 3, 5):
        for skip in (2, 3, 5):
            yield max_num, [(t == 0, (t % skip == 0) if skip > 2 else False, False) for t in range(40)]
            if max_num >= 2:                                   # (keyframes need a bank that can hold anchors)
                for every in (4, 7):
                    yield max_num, [(t == 0, (t % skip == 0) if skip > 2 else False, t > 0 and t % every == 0) for t in range(40)]
    yield 3, [(t % 9 == 0, t % 2 == 0, t % 9 == 5) for t in range(40)]          # several clips


def test_pending_applies_the_bank_policy_and_the_early_split_reunites():
    for max_num, frames in _schedules():
        bank, ref = [], []
        for t, (first, mem, anchor) in enumerate(frames):
            pend = Pending(dict(frame=t), "plan", t & 1, first, mem, max_num, anchor)
            new_ref = dict(frame=t)
            old, fresh = early_read_split(bank, pend)          # (before the memorize runs, as the frame step asks)
            nb, released = pend.apply(bank)
            ref, released_ref = bank_update(ref, new_ref, first, mem, max_num, anchor)
            assert [s["frame"] for s in nb] == [s["frame"] for s in ref]
            assert [s["frame"] for s in released] == [s["frame"] for s in released_ref]
            assert [bool(s.get("anchor")) for s in nb] == [bool(s.get("anchor")) for s in ref]
            # old + fresh is that bank, slot for slot; fresh is the new slot alone, and only where the policy keeps it
            assert len(old) + len(fresh) == len(nb) and all(any(s is k for k in old + fresh) for s in nb)
            assert fresh == ([pend.slot] if any(s is pend.slot for s in nb) else []) and not any(s is pend.slot for s in old)
            assert [s["frame"] for s in old] == [s["frame"] for s in nb if s is not pend.slot]
            bank = nb
        assert early_read_split(bank, None) == (bank, []) and early_read_split(bank, None)[0] is not bank


def _parent_decision(verdict, first_frame, rechecks, predict_off, predicted):
    """The branches of the frame step as they stood before the decision had a function of its own."""
    if predicted and not predict_off:
        if first_frame and verdict != "ok" and rechecks > 0:
            return DROP_RECOMPUTE if verdict == "off" else RECOMPUTE
        return WARN_SUSPECT if verdict == "off" and not first_frame else GO_ON
    if predict_off and predicted and first_frame:
        return DROP_RECOMPUTE
    return GO_ON


def test_retry_decision_full_table():
    table = list(itertools.product(("ok", "p3", "off"), (False, True), (0, 1, 2), (False, True), (False, True)))
    assert len(table) == 72
    for row in table:
        assert retry_decision(*row) == _parent_decision(*row), row
    # the rows that matter, spelled out: (verdict, first_frame, rechecks, gn_predict_off before the check, plan predicts)
    assert retry_decision("ok", True, 2, False, True) == GO_ON
    assert retry_decision("p3", True, 2, False, True) == RECOMPUTE
    assert retry_decision("off", True, 1, False, True) == DROP_RECOMPUTE
    assert retry_decision("p3", True, 0, False, True) == GO_ON and retry_decision("off", True, 0, False, True) == GO_ON
    assert retry_decision("off", False, 2, False, True) == WARN_SUSPECT
    assert retry_decision("p3", False, 2, False, True) == GO_ON
    assert retry_decision("ok", True, 2, True, True) == DROP_RECOMPUTE          # the guard tripped in the previous clip
    assert retry_decision("ok", True, 0, True, True) == DROP_RECOMPUTE          # (whatever is left: the recomputation gets none)
    assert retry_decision("ok", False, 2, True, True) == GO_ON
    assert all(retry_decision(v, f, 2, o, False) == GO_ON for v in ("ok", "p3", "off") for f in (False, True) for o in (False, True))
    assert {GO_ON, RECOMPUTE, DROP_RECOMPUTE, WARN_SUSPECT} == {"go on", "recompute", "drop plans and recompute", "warn suspect"}
