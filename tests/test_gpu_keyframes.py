"""GPU (-m gpu): keyframe trimaps -- the label kernel bit for bit, and clips with trimaps / label maps on several frames
against the composition of the oracle's own stages (tests/keyframe_ref.py), with the suite's tie-break protocol
(tests/test_gpu_frame.py: a class map that differs from the composition's may only differ at near-ties, and the composition
then goes on with the device's tie-breaks, so the 1e-3 alpha bound is always asserted)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ALPHA_TOL = 1e-3            # the project's contract (BASELINE.json)


@pytest.fixture(scope="module")
def model(synth_sd):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_gpu_frame import _fresh_model
    return _fresh_model(synth_sd, 12).module


def _label_ref(probs, labels, lh, lw):
    """numpy statement of otvm_trimap_apply_labels: planar probs [3,Hp,Wp], labels [H,W]."""
    out = probs.copy()
    H, W = labels.shape
    inner = out[:, lh:lh + H, lw:lw + W]
    has = labels != 255
    for c in range(3):
        inner[c][has] = (labels[has] == c).astype(np.float32)
    return out


@pytest.mark.parametrize("density", [0.0, 0.05, 1.0], ids=["none", "5pct", "all"])
@pytest.mark.parametrize("H,W", [(100, 150), (1080, 1920), (2160, 3840)], ids=["100x150", "1080p", "4k"])
def test_trimap_apply_labels_bit_for_bit(H, W, density):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from otvm_amd import lib as L
    from otvm_amd.engine import pad_amounts
    lib = L.load()
    lw, uw, lh, uh = pad_amounts(H, W, 32)
    Hp, Wp = H + lh + uh, W + lw + uw
    assert (Hp, Wp) == {(100, 150): (128, 160), (1080, 1920): (1088, 1920), (2160, 3840): (2176, 3840)}[(H, W)]
    rng = np.random.Generator(np.random.PCG64(H + int(100 * density)))
    probs = rng.standard_normal((3, Hp, Wp), dtype=np.float32)          # any bits: the kernel copies or overwrites, never computes
    labels = np.full((H, W), 255, np.uint8)
    if density > 0:
        has = rng.random((H, W)) < density if density < 1 else np.ones((H, W), bool)
        labels[has] = rng.integers(0, 3, int(has.sum()), dtype=np.uint8)
    if density == 0.05:
        labels[0, :7] = (0, 1, 2, 255, 2, 1, 0)                         # the corner groups, whatever the draw
        labels[H - 1, W - 3:] = (2, 255, 1)
    pd = torch.from_numpy(probs).cuda()
    ld = torch.from_numpy(labels).cuda()
    L.check(lib.otvm_trimap_apply_labels(pd.data_ptr(), ld.data_ptr(), H, W, Hp, Wp, lh, lw, torch.cuda.current_stream().cuda_stream),
            "trimap_apply_labels")
    torch.cuda.synchronize()
    got = pd.cpu().numpy()
    want = _label_ref(probs, labels, lh, lw)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    border = np.ones((Hp, Wp), bool)
    border[lh:lh + H, lw:lw + W] = False
    assert np.array_equal(got[:, border].view(np.uint32), probs[:, border].view(np.uint32))      # the padding border is untouched
    if density == 0.0:
        assert np.array_equal(got.view(np.uint32), probs.view(np.uint32))


def _clip(H, W, T, seed):
    """Frames (uint8 BGR) of a seeded synthetic clip, a trimap for any of its frames (the clip's disc moves by (0.5, 1) pixels
    per frame: the first-frame trimap shifted along) and a label map for any frame: ~5 % of the pixels -- the disc's core as
    foreground, the top rows as background, a thin ring as unknown."""
    from otvm_amd.synth_data import synthetic_clip
    frames, tri = synthetic_clip(H, W, T, seed=seed)

    def tri_at(t):
        return np.ascontiguousarray(np.roll(tri, (int(0.5 * t), t), axis=(1, 2)))

    def labels_at(t):
        yy, xx = np.mgrid[0:H, 0:W]
        r = np.sqrt((yy - H / 2 - 0.5 * t) ** 2 + (xx - W / 2 - 1.0 * t) ** 2)
        lab = np.full((H, W), 255, np.uint8)
        lab[r < H / 10] = 2
        lab[:2, :] = 0
        lab[np.abs(r - 0.29 * H) < 0.6] = 1
        return lab
    return frames, tri_at, labels_at


def _matte_against_composition(m, sd, frames, keyframes, skip, max_num, label):
    """run_video_matte(keyframes=...) with the composition stepped alongside (on_frame fires in schedule order).  Prints every
    figure before anything is asserted; returns (result, per-step log)."""
    from otvm_amd.video import memory_schedule, run_video_matte
    from tests.keyframe_ref import KeyframeComposition, schedule
    T = len(frames)
    H, W = frames[0].shape[:2]
    _, max_eff, large = memory_schedule(0, H, W, skip, max_num)
    kinds = {t: ("key" if np.asarray(v).ndim == 3 else "labels") for t, v in keyframes.items()}
    steps = schedule(T, kinds, skip * 2 if large else skip)
    k0 = steps[0][0]
    comp = KeyframeComposition(sd, dilate_kernel=12)
    eng_of = m
    it, log = iter(steps), []

    def on_frame(i, alpha, u8, out):
        torch.cuda.synchronize()
        t, kind, first, last, mem = next(it)
        assert t == i, (t, i)
        eng = eng_of._engine
        pl = eng.last_plan
        cls_h = pl.CLS.reshape(pl.Hp, pl.Wp).cpu().long()
        if t == k0 - 1:
            comp.drop_non_anchors()
        fg = torch.from_numpy(frames[t].astype(np.float32)).permute(2, 0, 1)[None].contiguous()
        r = comp.step(fg, t, kind, first, last, mem, max_eff, tri=keyframes[t] if kind == "key" else None,
                      labels=keyframes[t] if kind == "labels" else None, cls_hip=cls_h)
        d = float((alpha.cpu() - r["alpha"]).abs().max())
        mem_now = eng_of.memories
        rec = dict(t=t, kind=kind, d=d, ties=r["ties"], T_read=eng.last_T_read, ref_T_read=r["T_read"], bank=mem_now["frames"],
                   anchors=mem_now["anchors"], ref_bank=comp.frames(), ref_anchors=comp.anchors(),
                   cls=cls_h[pl.lh:pl.lh + H, pl.lw:pl.lw + W].numpy())
        print("%s step %d: frame %d (%s) alpha max-abs %.3e, tie-breaks %d, T_read %d, bank %s anchors %s | composition bank %s "
              "anchors %s" % (label, len(log), t, kind, d, r["ties"], rec["T_read"], rec["bank"], rec["anchors"], rec["ref_bank"],
                              rec["ref_anchors"]))
        log.append(rec)
    res = run_video_matte(m, frames, keyframes=keyframes, skip=skip, max_num=max_num, on_frame=on_frame)
    assert [tuple(s) for s in res["schedule"]] == steps
    return res, log


def _assert_clip(res, log, keyframes, T):
    assert sorted(r["t"] for r in log) == list(range(T))
    for r in log:
        t = r["t"]
        assert r["d"] <= ALPHA_TOL, "frame %d (%s): alpha max-abs %.3e vs the composition" % (t, r["kind"], r["d"])
        assert r["bank"] == r["ref_bank"] and r["anchors"] == r["ref_anchors"], (t, r["bank"], r["ref_bank"], r["anchors"])
        assert r["T_read"] == r["ref_T_read"], (t, r["T_read"], r["ref_T_read"])
        if r["kind"] == "key":
            assert r["T_read"] == 0                               # a full keyframe reads no memory
        else:
            assert r["T_read"] >= 1
        if r["kind"] == "labels":
            lab = keyframes[t]
            has = lab != 255
            assert has.any() and np.array_equal(r["cls"][has], lab[has].astype(np.int64))
        assert res["bank_frames"][t] == r["bank"] and res["anchor_frames"][t] == r["anchors"]
    assert res["alpha"].shape[0] == T and res["alpha_u8"].shape[0] == T
    assert torch.equal(res["alpha_u8"], (res["alpha"] * 255).to(torch.uint8))       # natural order, one frame each


def test_clip_with_two_keyframes_and_a_correction(model, synth_sd):
    """100x150, 8 frames, memory every 3 / at most 3: trimaps on frames 0 and 5, a label map on frame 3."""
    H, W, T = 100, 150, 8
    frames, tri_at, labels_at = _clip(H, W, T, seed=41)
    kf = {0: tri_at(0), 5: tri_at(5), 3: labels_at(3)}
    res, log = _matte_against_composition(model, synth_sd, frames, kf, 3, 3, "keyframes {0,5}+labels 3")
    _assert_clip(res, log, kf, T)
    assert [r["t"] for r in log] == [0, 5, 1, 2, 3, 4, 6, 7]
    assert all(set(r["anchors"]) <= {0, 5} and 0 in r["anchors"] for r in log)
    assert all(r["anchors"] == [0, 5] for r in log[1:-1])          # both anchors resident from the second step on
    assert max(len(r["bank"]) for r in log) == 4                   # max_memory_num + one extra anchor


def test_clip_with_a_mid_clip_trimap_only(model, synth_sd):
    """The same clip with its only trimap on frame 3: frames 4..7 come from the forward sweep, 2, 1, 0 from the backward one
    (which starts from the anchor alone); a label map on frame 1 is applied in the backward sweep."""
    H, W, T = 100, 150, 8
    frames, tri_at, labels_at = _clip(H, W, T, seed=41)
    kf = {3: tri_at(3), 1: labels_at(1)}
    res, log = _matte_against_composition(model, synth_sd, frames, kf, 3, 3, "keyframe {3}")
    _assert_clip(res, log, kf, T)
    assert [r["t"] for r in log] == [3, 4, 5, 6, 7, 2, 1, 0]
    assert log[5]["T_read"] == 1 and log[5]["bank"] == [3, 2]      # the backward sweep read the anchor alone
    assert all(r["anchors"] == [3] for r in log)


def test_mirror_property(model):
    """A clip matted with {k: trimap} and its time reversal matted with {T-1-k: trimap} are the same computation: equal bits,
    frame for frame in reversed order (one process, one tune cache)."""
    from otvm_amd.video import run_video_matte
    H, W, T, k = 100, 150, 8, 3
    frames, tri_at, _ = _clip(H, W, T, seed=43)
    fwd = run_video_matte(model, frames, keyframes={k: tri_at(k)}, skip=3, max_num=3)
    rev = run_video_matte(model, np.ascontiguousarray(frames[::-1]), keyframes={T - 1 - k: tri_at(k)}, skip=3, max_num=3)
    assert [s[0] for s in fwd["schedule"]] == [3, 4, 5, 6, 7, 2, 1, 0] and [s[0] for s in rev["schedule"]] == [4, 5, 6, 7, 3, 2, 1, 0]
    for t in range(T):
        same = torch.equal(fwd["alpha"][t], rev["alpha"][T - 1 - t])
        print("mirror: frame %d %s" % (t, "equal" if same else "differs by %.3e" % float((fwd["alpha"][t] - rev["alpha"][T - 1 - t]).abs().max())))
    for t in range(T):
        assert torch.equal(fwd["alpha"][t], rev["alpha"][T - 1 - t]), t
        assert torch.equal(fwd["trimap"][t], rev["trimap"][T - 1 - t]), t


def test_first_frame_trimap_alone_is_unchanged(model):
    """run_video_matte(trimap=X) and run_video_matte(keyframes={0: X}): equal bits, equal launches per frame, equal digest."""
    from otvm_amd.engine import kernel_config_digest
    from otvm_amd.video import run_video_matte
    H, W, T = 100, 150, 8
    frames, tri_at, _ = _clip(H, W, T, seed=44)
    run_video_matte(model, frames[:2], trimap=tri_at(0), skip=3, max_num=3)       # plans built and tuned before anything is counted
    eng = model._engine

    def run(**kw):
        counts, last = [], [eng.conv_calls]

        def on_frame(i, alpha, u8, out):
            counts.append((i, eng.conv_calls - last[0], eng.last_T_read))
            last[0] = eng.conv_calls
        res = run_video_matte(model, frames, skip=3, max_num=3, on_frame=on_frame, **kw)
        return res, counts, kernel_config_digest()
    a, ca, da = run(trimap=tri_at(0))
    b, cb, db = run(keyframes={0: tri_at(0)})
    print("launches per frame (frame, convolution launches, T_read):", ca)
    assert ca == cb and da == db
    assert torch.equal(a["alpha"], b["alpha"]) and torch.equal(a["alpha_u8"], b["alpha_u8"]) and torch.equal(a["trimap"], b["trimap"])
    assert a["bank_frames"] == b["bank_frames"]
    assert sorted(a) == ["alpha", "alpha_u8", "bank_frames", "trimap"]          # the result of a call without keyframes keeps its keys
    assert b["anchor_frames"] == [[0]] * T and [st[0] for st in b["schedule"]] == list(range(T))


def test_frame_step_refusals(model):
    H, W = 100, 150
    frames, tri_at, labels_at = _clip(H, W, 2, seed=45)
    fg = torch.from_numpy(frames[0]).cuda()
    a, tg = torch.ones(1, 1, 1, H, W, device="cuda"), torch.from_numpy(tri_at(0))[None, None].cuda()
    lab = torch.from_numpy(labels_at(0)).cuda()
    with pytest.raises(ValueError):
        model(a, fg, fg, tri_gt=tg, first_frame=True, labels=lab, max_memory_num=3)
    model(a, fg, fg, tri_gt=tg, first_frame=True, max_memory_num=3)
    with pytest.raises(ValueError):
        model(a, fg, fg, tri_gt=None, keyframe=True, max_memory_num=3)
    with pytest.raises(ValueError):
        model(a, fg, fg, tri_gt=tg, keyframe=True, max_memory_num=1)
    with pytest.raises(ValueError):
        model(a, fg, fg, tri_gt=tg, labels=lab, max_memory_num=0)
    with pytest.raises(NotImplementedError):
        model.forward_batch([a], [fg], [fg], [tg], keyframe=True)
    model(a, fg, fg, tri_gt=tg, last_frame=True, max_memory_num=3)               # the clip is still intact
    torch.cuda.synchronize()


def test_1080p_keyframe_and_correction_vs_composition(model, synth_sd):
    """One frame pair at BASELINE configs[2]'s geometry (1920x1080 -> 1088x1920): three frames, the trimap on frame 1, a label
    map on frame 2; frame 0 comes from the backward sweep.  Three CPU oracle frames."""
    H, W, T = 1080, 1920, 3
    frames, tri_at, labels_at = _clip(H, W, T, seed=46)
    kf = {1: tri_at(1), 2: labels_at(2)}
    res, log = _matte_against_composition(model, synth_sd, frames, kf, 3, 3, "1080p keyframe {1}+labels 2")
    _assert_clip(res, log, kf, T)
    assert [r["t"] for r in log] == [1, 2, 0]


def test_eval_cli_keyframes_on_a_demo_tree(tmp_path, model):
    """eval_cli --demo --keyframes on a synthetic demo tree whose first frame has NO trimap (trimaps on frames 1 and 4, a label
    map on frame 3): a PNG per frame, byte-equal to run_video_matte on the decoded clip."""
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.datasets import Demo_Test, load_sequence
    from otvm_amd.video import run_video_matte
    H, W, T = 100, 150, 6
    frames, tri_at, labels_at = _clip(H, W, T, seed=47)
    root = os.path.join(str(tmp_path), "demo")
    for d in ("frames", "trimap", "labels"):
        os.makedirs(os.path.join(root, "clip", d))
    for t in range(T):
        Image.fromarray(frames[t][..., ::-1].copy()).save(os.path.join(root, "clip", "frames", "%05d.png" % t))
    for t in (1, 4):
        tri = tri_at(t)
        Image.fromarray((tri[1] * 128 + tri[2] * 255).astype(np.uint8)).save(os.path.join(root, "clip", "trimap", "%05d.png" % t))
    lab = labels_at(3)
    grey = np.full((H, W), 64, np.uint8)                       # 64: not a class level -> unlabelled
    for cls, level in ((0, 0), (1, 128), (2, 255)):
        grey[lab == cls] = level
    Image.fromarray(grey).save(os.path.join(root, "clip", "labels", "00003.png"))
    out_dir = os.path.join(str(tmp_path), "results")
    s = eval_cli.main(["--demo", "--data", root, "--out", out_dir, "--synthetic-weights", "--keyframes", "--skip", "3",
                       "--max-num", "3"])
    assert s["frames"] == T
    d = load_sequence(next(iter(Demo_Test(root))), keyframes=True)
    assert sorted(d["keyframe_trimaps"]) == [1, 4] and sorted(d["label_maps"]) == [3]
    assert np.array_equal(d["keyframe_trimaps"][4], tri_at(4)) and np.array_equal(d["label_maps"][3], lab)
    assert all(np.array_equal(d["frames"][t], frames[t]) for t in range(T))
    direct = run_video_matte(model, d["frames"], keyframes={**d["keyframe_trimaps"], **d["label_maps"]}, skip=3, max_num=3)
    assert [st[0] for st in direct["schedule"]] == [1, 4, 2, 3, 5, 0]
    pred = os.path.join(out_dir, "alpha", "test", "s4_OTVM", "pred", "clip")
    assert sorted(os.listdir(pred)) == ["%05d.png" % t for t in range(T)]
    for t in range(T):
        png = np.asarray(Image.open(os.path.join(pred, "%05d.png" % t)))
        assert png.shape == (H, W) and np.array_equal(png, direct["alpha_u8"][t].numpy()), t
    assert torch.equal(s["outputs"][0]["alpha"].cpu(), direct["alpha"])
    # without the flag the extra files are ignored -- and this clip, whose first frame has no trimap, is refused as before
    with pytest.raises(FileNotFoundError):
        eval_cli.main(["--demo", "--data", root, "--out", out_dir + "_plain", "--synthetic-weights"])
