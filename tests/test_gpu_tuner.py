"""GPU (-m gpu): the plan-time tuner end to end on a small frame -- what it logs, how many conv launches it counts, and that a
second engine fed the tune file it wrote times nothing and mattes the same bits.  (The protocol and the ladder themselves are
tested on the CPU: tests/test_tuner_cpu.py.)"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK, UPFOLD = " (fused bottleneck:", " (2x upsampling:"


def test_tuned_plan_logs_counts_and_reloads(synth_sd, tmp_path, monkeypatch):
    """A 96x128 frame is padded to itself; its 1/16-resolution maps are 6x8; the plan has planes-128 STM blocks and both decoder
    maps.  conv_calls after the plan was built is DERIVED from the protocol: 3 + 4 * (codes + 1) per conv signature, 42 per
    planes-128 block, 28 per reader of an upsampled map.  (Measured once on an MI355X, the parent commit and this one: 60 conv
    signatures, 1 planes-128 map and 1 upsampled map with 2 readers timed, 9098 launches counted by both.  The library folds the
    map at this size, so no larger frame is needed; the test recomputes the sum from the log of its own run.)"""
    from otvm_amd import engine, helpers
    from otvm_amd.synth_data import synthetic_clip
    from otvm_amd.video import run_video_matte
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    H, W = 96, 128
    monkeypatch.setattr(engine, "_TUNE_CACHE", {})
    monkeypatch.setattr(engine, "TUNE_FILE", str(tmp_path / "tune.json"))
    monkeypatch.setattr(engine, "AUTOTUNE", True)
    monkeypatch.setattr(engine, "FUSE_STM_BLOCK128", 1)
    monkeypatch.setattr(engine, "FOLD_UPSAMPLE", 1)
    frames, tri = synthetic_clip(H, W, 3, seed=321)
    cfg = helpers.default_cfg()

    def fresh_engine():
        m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
        m.load_state_dict(synth_sd, strict=True)
        m = m.cuda().eval()
        return m, m._get_engine()

    def matte(m):
        return run_video_matte(m, frames, trimap=tri, skip=2, max_num=3)

    # ---- first engine: everything is timed
    m1, e1 = fresh_engine()
    n0, c0 = len(engine.TUNE_LOG), e1.conv_calls
    pl1 = e1.plan(H, W)
    tuned_calls = e1.conv_calls - c0
    new = engine.TUNE_LOG[n0:]
    blocks = [t for t in new if BLOCK in t[0]]
    upfolds = [t for t in new if UPFOLD in t[0]]
    convs = [t for t in new if BLOCK not in t[0] and UPFOLD not in t[0]]
    print("timed: %d conv signatures, %d planes-128 maps, %d upsampled maps; %d conv launches" % (
        len(convs), len(blocks), len(upfolds), tuned_calls))
    assert convs and blocks and upfolds
    for name, sig, choice, ms in convs:
        assert 0 in ms and choice in ms and all(math.isfinite(t) and t > 0 for t in ms.values()), (name, ms)
    for name, sig, choice, ms in blocks:
        assert set(ms) == {0, 1, 2, 3} and choice in ms and all(math.isfinite(t) and t > 0 for t in ms.values()), (name, ms)
    for name, sig, choice, ms in upfolds:
        assert set(ms) == {0, 1} and choice in ms and all(math.isfinite(t) and t > 0 for t in ms.values()), (name, ms)
    # the launches the protocol implies
    upfold_keys = [k for k in engine._TUNE_CACHE if k[0] == -2]
    assert len(upfold_keys) == len(upfolds) and all((len(k) - 6) % 3 == 0 and len(k) > 6 for k in upfold_keys)
    readers = sum((len(k) - 6) // 3 for k in upfold_keys)
    assert tuned_calls == sum(3 + 4 * (len(ms) + 1) for _, _, _, ms in convs) + 42 * len(blocks) + 28 * readers
    assert len(engine._TUNE_CACHE) == len(new)                   # every timed choice is stored, under a key of its own
    c1 = e1.conv_calls
    a = matte(m1)
    frame_calls = e1.conv_calls - c1
    assert len(engine.TUNE_LOG) == n0 + len(new) and frame_calls > 0     # the frames found every shape in the cache
    routes1, saved = dict(pl1.upfold_routes), dict(engine._TUNE_CACHE)
    # one time per candidate offered, every conv entry (the frames bound the key / value convs, timed on scratch blocks, to slots)
    offered = {}
    codes = (C.c_int * 128)()
    for p, name in pl1._convs:
        n = int(pl1.lib.otvm_conv2d_candidates(C.byref(p), codes, 128))
        offered[pl1._signature(p)] = {0} | {int(codes[i]) for i in range(n) if engine.WAVE_TILE or int(codes[i]) // 16 - 1 != 9}
    for name, sig, choice, ms in convs:
        assert set(ms) == offered[sig], (name, ms, offered[sig])

    # ---- second engine, from the file the first one wrote: nothing is timed
    engine._TUNE_CACHE.clear()
    engine._load_tune_file()
    assert engine._TUNE_CACHE == saved
    m2, e2 = fresh_engine()
    c0 = e2.conv_calls
    pl2 = e2.plan(H, W)
    assert e2.conv_calls == c0 and len(engine.TUNE_LOG) == n0 + len(new)
    assert pl2.upfold_routes == routes1 and {"NET.decoder.conv_up2.1", "NET.decoder.conv_up3.1"} <= set(routes1)
    b = matte(m2)
    assert e2.conv_calls - c0 == frame_calls and len(engine.TUNE_LOG) == n0 + len(new)
    assert torch.equal(a["alpha"], b["alpha"]) and torch.equal(a["trimap"], b["trimap"])
