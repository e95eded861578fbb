"""Keyframe trimaps, host side (no GPU): the anchor-aware bank policy, the offline schedule, the discovery of trimap/ and
labels/ files in the demo layout, and the new symbol / arguments."""
import inspect
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_equals_the_reference_with_one_anchor():
    """With the first frame as the only anchor the policy is alpha/model.py:472-493: every memorize pattern of up to 8 frames,
    max_memory_num 0..5, the frame ids after every step against the oracle's restatement of the reference."""
    from oracle.otvm_oracle import bank_update as orc_update
    from otvm_amd.engine import bank_update
    n = 0
    for max_num in range(6):
        for length in range(1, 9):
            for pattern in itertools.product((False, True), repeat=length):
                eb, ob = [], []
                for t, mem in enumerate(pattern):
                    eb, released = bank_update(eb, dict(frame=t), t == 0, mem, max_num)
                    ob = orc_update(ob, (None, None, t), t == 0, mem, max_num)
                    assert [s["frame"] for s in eb] == [b[2] for b in ob], (max_num, pattern, t)
                    assert all(not any(r is k for k in eb) for r in released)
                n += 1
    assert n == 6 * (2 ** 9 - 2)


def test_policy_with_extra_anchors():
    """Random schedules (fixed seed): anchors never leave before the next first_frame, the bank never exceeds
    max_memory_num + (anchors - 1), slots stay in insertion order, the released list is exactly what left the bank -- and the
    frame ids equal the independent restatement of tests/keyframe_ref.py."""
    from otvm_amd.engine import bank_update
    from tests.keyframe_ref import Slot, anchor_policy
    rng = np.random.Generator(np.random.PCG64(7))
    for trial in range(200):
        max_num = int(rng.integers(2, 6))
        bank, rbank, anchors = [], [], []
        for t in range(int(rng.integers(5, 60))):
            first = t == 0 or rng.random() < 0.02
            anchor = bool(rng.random() < 0.15)
            mem = bool(rng.random() < 0.3)
            new = dict(frame=t, anchor=not anchor)          # (a stale flag of a recycled slot must not count)
            before = list(bank)
            bank, released = bank_update(bank, new, first, mem, max_num, anchor=anchor)
            rbank = anchor_policy(rbank, Slot(None, None, t, first or anchor), first, mem, max_num)
            anchors = [t] if first else anchors + ([t] if anchor else [])
            ids = [s["frame"] for s in bank]
            assert ids == [s.frame for s in rbank], (trial, t, ids)
            assert [s["frame"] for s in bank if s["anchor"]] == anchors == [s.frame for s in rbank if s.anchor], (trial, t)
            assert len(bank) <= max_num + len(anchors) - 1
            assert ids == sorted(ids) and len(set(ids)) == len(ids)
            left = [s for s in before + [new] if not any(s is k for k in bank)]
            assert len(released) == len(left) and all(a is b for a, b in zip(released, left))
            assert all(any(s is k for k in before + [new]) for s in bank)


def test_schedule():
    from otvm_amd.video import keyframe_schedule
    from tests.keyframe_ref import schedule as ref_schedule
    # {0: ...} is eval.py:178-189
    for T in range(1, 26):
        for skip in (1, 2, 3, 5, 10):
            steps = keyframe_schedule(T, {0: "key"}, skip)
            want = [(t, "key" if t == 0 else "frame", t == 0, t == T - 1, (t % skip == 0) if skip > 2 else False) for t in range(T)]
            assert steps == want, (T, skip)
    rng = np.random.Generator(np.random.PCG64(3))
    for trial in range(300):
        T = int(rng.integers(1, 30))
        skip = int(rng.choice([1, 2, 3, 5, 10]))
        kinds = {int(t): ("key" if rng.random() < 0.5 else "labels") for t in rng.choice(T, size=int(rng.integers(1, min(T, 6) + 1)),
                                                                                     replace=False)}
        kinds[int(rng.integers(0, T))] = "key"
        steps = keyframe_schedule(T, kinds, skip)
        assert sorted(s[0] for s in steps) == list(range(T))                     # every frame exactly once
        keys = sorted(t for t, k in kinds.items() if k == "key")
        k0 = keys[0]
        assert steps[0][0] == k0 and steps[0][2] and [s[2] for s in steps].count(True) == 1
        assert [s[0] for s in steps[:len(keys)]] == keys and all(s[1] == "key" for s in steps[:len(keys)])
        assert [s[3] for s in steps].count(True) == 1 and steps[-1][3]
        assert all(s[1] == kinds.get(s[0], "frame") for s in steps)
        rest = [s[0] for s in steps[len(keys):]]
        fwd = [t for t in range(k0 + 1, T) if t not in keys]
        assert rest == fwd + list(range(k0 - 1, -1, -1))
        assert all(s[4] == ((abs(s[0] - k0) % skip == 0) if skip > 2 else False) for s in steps)
        assert steps == ref_schedule(T, kinds, skip)
    # arrays classify themselves: [3,H,W] a trimap, [H,W] a label map
    steps = keyframe_schedule(4, {2: np.zeros((3, 4, 4), np.float32), 1: np.zeros((4, 4), np.uint8)}, 3)
    assert [(s[0], s[1]) for s in steps] == [(2, "key"), (3, "frame"), (1, "labels"), (0, "frame")]
    with pytest.raises(ValueError):
        keyframe_schedule(5, {2: "labels"}, 3)                                   # no full keyframe
    with pytest.raises(ValueError):
        keyframe_schedule(5, {}, 3)
    with pytest.raises(ValueError):
        keyframe_schedule(5, {0: "key", 5: "key"}, 3)                            # outside the clip
    with pytest.raises(ValueError):
        keyframe_schedule(5, {-1: "key"}, 3)


def test_demo_layout_discovery(tmp_path):
    from PIL import Image
    from otvm_amd.datasets import Demo_Test, load_sequence
    from otvm_amd.synth_data import disc_trimap
    H, W, T = 12, 16, 6
    root = str(tmp_path)
    for d in ("frames", "trimap", "labels"):
        os.makedirs(os.path.join(root, "clip", d))
    rng = np.random.Generator(np.random.PCG64(1))
    for t in range(T):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "clip", "frames", "%05d.png" % t))
    tri = disc_trimap(H, W)
    g = (tri[1] * 128 + tri[2] * 255).astype(np.uint8)
    for t in (0, 4):
        Image.fromarray(np.roll(g, t, axis=1)).save(os.path.join(root, "clip", "trimap", "%05d.png" % t))
    lab = np.full((H, W), 77, np.uint8)                       # 77, 1, 254: not a class -> unlabelled
    lab[0, :4] = (0, 128, 255, 254)
    lab[1, :2] = (1, 127)
    Image.fromarray(lab).save(os.path.join(root, "clip", "labels", "00002.png"))
    item = next(iter(Demo_Test(root)))
    assert len(item) == 7 and item[0] == "demo"               # the 7-tuple protocol is unchanged
    assert item[5] == ["clip/trimap/00000.png"] * 4 + ["clip/trimap/00004.png"] * 2
    plain = load_sequence(item)
    assert "keyframe_trimaps" not in plain and "label_maps" not in plain       # without the flag: ignored, as before
    assert np.array_equal(plain["trimap"], tri)
    keyed = load_sequence(item, keyframes=True)
    assert sorted(keyed["keyframe_trimaps"]) == [0, 4] and sorted(keyed["label_maps"]) == [2]
    assert np.array_equal(keyed["keyframe_trimaps"][0], tri) and np.array_equal(keyed["trimap"], tri)
    assert np.array_equal(keyed["keyframe_trimaps"][4], np.roll(tri, 4, axis=2))
    want = np.full((H, W), 255, np.uint8)
    want[0, :3] = (0, 1, 2)
    assert keyed["label_maps"][2].dtype == np.uint8 and np.array_equal(keyed["label_maps"][2], want)
    assert len(keyed["frames"]) == T and keyed["names"] == ["%05d" % t for t in range(T)]
    # a clip whose FIRST frame has no trimap: refused without the flag (as before), fine with it
    os.remove(os.path.join(root, "clip", "trimap", "00000.png"))
    item = next(iter(Demo_Test(root)))
    with pytest.raises(FileNotFoundError):
        load_sequence(item)
    keyed = load_sequence(item, keyframes=True)
    assert sorted(keyed["keyframe_trimaps"]) == [4] and keyed["trimap"] is None
    assert load_sequence(item, keyframes=True, max_frames=5)["keyframe_trimaps"].keys() == {4}
    with pytest.raises(FileNotFoundError):
        load_sequence(item, keyframes=True, max_frames=3)     # no trimap among the frames kept


def test_library_exports_the_label_kernel_and_keeps_abi_21():
    from otvm_amd.csrc.build import build
    from otvm_amd import lib as L
    build()
    h = L.load()
    assert "otvm_trimap_apply_labels" in L.EXPORTED and h.otvm_trimap_apply_labels is not None
    assert h.otvm_abi_version() == 21 and L.ABI_VERSION == 21
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    assert "int otvm_trimap_apply_labels(float* probs, const uint8_t* labels, int H, int W, int Hp, int Wp, int lh, int lw," in header
    # bad arguments are refused on the host, before any launch (no GPU needed)
    assert h.otvm_trimap_apply_labels(None, None, 4, 4, 32, 32, 0, 0, None) != 0
    assert h.otvm_trimap_apply_labels(16, 16, 4, 4, 32, 32, 30, 0, None) != 0        # does not fit the padded frame
    assert h.otvm_trimap_apply_labels(16, 16, 4, 4, 32, 30, 0, 0, None) != 0        # padded width not a multiple of 4
    assert h.otvm_trimap_apply_labels(20, 16, 4, 4, 32, 32, 0, 0, None) != 0        # planes not 16-byte aligned
    assert b"otvm_trimap_apply_labels" in h.otvm_last_error()


def test_drivers_accept_the_keyframe_arguments(monkeypatch):
    from otvm_amd import eval_cli, video
    from otvm_amd.alpha_model import EvalModel
    sig = inspect.signature(EvalModel.forward)
    assert sig.parameters["keyframe"].default is False and sig.parameters["labels"].default is None
    assert list(sig.parameters)[:11] == ["self", "a", "fg", "bg", "tri", "tri_gt", "first_frame", "last_frame", "memorize",
                                         "max_memory_num", "large_input"]    # the reference's surface, in its order
    assert inspect.signature(video.run_video_matte).parameters["keyframes"].default is None
    assert inspect.signature(video.run_video_matte_batch).parameters["keyframes"].default is None
    with pytest.raises(NotImplementedError):
        video.run_video_matte_batch(None, [[None]], trimaps=[None], keyframes={0: "key"})
    with pytest.raises(NotImplementedError):
        EvalModel.forward_batch(None, [], [], [], [], keyframe=True)
    with pytest.raises(NotImplementedError):
        EvalModel.forward_batch(None, [], [], [], [], labels=np.zeros((2, 2), np.uint8))
    assert hasattr(EvalModel, "drop_non_anchors")
    seen = {}

    class Stop(Exception):
        pass
    import argparse
    orig = argparse.ArgumentParser.parse_args

    def spy(self, argv=None):
        ns = orig(self, argv)
        seen.update(vars(ns))
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(Stop):
        eval_cli.main(["--demo", "--data", "x", "--keyframes"])
    assert seen["keyframes"] is True
    with pytest.raises(Stop):
        eval_cli.main(["--demo", "--data", "x"])
    assert seen["keyframes"] is False
