"""GPU (-m gpu): the training-mode forward (forward only) -- loss kernels against the oracle's restatement
of utils/loss_func.py, and FullModel.forward against the CPU oracle and the reference-generated fixtures; then every entry of
csrc/losses.hip on its own, accumulator by accumulator, against the float64 terms of tests/train_loss_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_loss_kernels_vs_oracle_functions():
    """csrc/losses.hip through the C ABI against oracle/train_oracle.py's functions (= utils/loss_func.py) on random data."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import train_oracle as T
    from otvm_amd import lib as L
    from otvm_amd.train import _fba_loss
    lib = L.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    B, S, H, W = 2, 3, 64, 96
    pred = torch.rand(B, S, 7, H, W, generator=g)
    gts = torch.rand(B, S, 1, H, W, generator=g)
    gts[gts < 0.3] = 0.0
    gts[gts > 0.8] = 1.0
    tm = (torch.rand(B, S, 1, H, W, generator=g) > 0.5).float()
    fgs, bgs, imgs = (torch.rand(B, S, 3, H, W, generator=g) for _ in range(3))
    want = T.fba_loss(pred, tm, gts, fgs, bgs, imgs)
    got = _fba_loss(lib, st, dev, *(x.to(dev).contiguous() for x in (pred, gts, tm, fgs, bgs, imgs)), B, S, H, W)
    for i, name in enumerate(("L_alpha_comp", "L_lap", "L_grad")):
        assert abs(got[i] - float(want[i])) <= 2e-5 * max(1.0, abs(float(want[i]))), (name, got[i], float(want[i]))
    for i, name in ((3, "alphas"), (4, "comps"), (5, "Fs"), (6, "Bs")):
        assert float((got[i].cpu() - want[i]).abs().max()) <= 1e-6, name
    # cross-entropy, trimask, scale / flip
    lg = torch.randn(5, 3, H, W, generator=g) * 8
    tri = torch.rand(5, 3, H, W, generator=g)
    mask, vis = torch.empty(5, H, W, device=dev), torch.empty(5, H, W, device=dev)
    cls = torch.empty(5, H, W, dtype=torch.uint8, device=dev)
    gt5 = torch.rand(5, H, W, generator=g)
    tri_d, gt5_d, lg_d = tri.to(dev), gt5.to(dev), lg.to(dev)        # (kept alive: the raw pointers go to the C ABI)
    L.check(lib.otvm_trimask(tri_d.data_ptr(), 5, H * W, mask.data_ptr(), cls.data_ptr(), gt5_d.data_ptr(), vis.data_ptr(), st))
    assert torch.equal(cls.cpu().long(), tri.max(dim=1)[1]) and torch.equal(mask.cpu(), (tri.max(dim=1)[1] == 1).float())
    assert torch.equal(vis.cpu(), torch.where(mask.cpu().bool(), torch.ones_like(gt5) * 128 * (1. / 255), gt5))
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    L.check(lib.otvm_loss_ce3(lg_d.data_ptr(), cls.data_ptr(), 5, H * W, acc.data_ptr(), st))
    want_ce = float(F.cross_entropy(lg, tri.max(dim=1)[1]))
    assert abs(float(acc[0]) / (5 * H * W) - want_ce) <= 2e-5 * want_ce
    x = torch.rand(4, 3, H, W, generator=g) * 255
    y = torch.empty(4, 3, H, W, device=dev)
    x_d = x.to(dev)
    L.check(lib.otvm_scale_flip3(x_d.data_ptr(), 4, H * W, 1.0 / 255, y.data_ptr(), st))
    assert torch.equal(y.cpu(), x.flip([1]) * (1.0 / 255))


@pytest.mark.parametrize("name", ["b2_s3_64x64", "b1_s4_64x96"])
def test_training_forward_vs_oracle_and_reference_fixture(name, synth_sd):
    """FullModel.forward (models/alpha/model.py:189-312) on the HIP path: B clips in lock-step through the batched kernels, every
    frame memorised, frame 0 with the ground-truth trimap; the four losses within 1e-3 (relative) of the CPU oracle and of the
    reference's own outputs, the returned tensors within 1e-3."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle.otvm_oracle import OtvmOracle
    from oracle.train_oracle import train_forward as oracle_forward
    from otvm_amd import helpers
    from otvm_amd.synth_data import train_batch
    g = np.load(os.path.join(GOLDEN, "train_%s.npz" % name))
    B, S, H, W, seed = (int(g[k]) for k in ("B", "S", "H", "W", "seed"))
    a, fg, bg, tri = (torch.from_numpy(x) for x in train_batch(B, S, H, W, seed))
    cfg = helpers.default_cfg()
    m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Train", None), "Train", None)
    m.load_state_dict(synth_sd, strict=True)
    m = m.cuda().eval()
    out = m(a.cuda(), fg.cuda(), bg.cuda(), tri=tri.cuda())
    torch.cuda.synchronize()
    ref = oracle_forward(OtvmOracle(synth_sd), a, fg, bg, tri)
    names = ("loss1", "loss2", "loss3", "loss_trimap", "scaled_imgs", "tris_vis", "alphas", "comps", "scaled_gts", "Fs", "Bs", "preds_trimap")
    got = dict(zip(names, out))
    for k in ("loss1", "loss2", "loss3", "loss_trimap"):
        v, wo, wg = float(got[k]), float(ref[k]), float(g[k])
        print("%s %s: hip %.6f oracle %.6f reference %.6f" % (name, k, v, wo, wg))
        assert abs(v - wo) <= 1e-3 * max(1.0, abs(wo)) and abs(v - wg) <= 1e-3 * max(1.0, abs(wg)), (k, v, wo, wg)
    for k in ("alphas", "comps", "Fs", "Bs", "preds_trimap", "scaled_imgs", "tris_vis", "scaled_gts"):
        d = float((got[k].cpu() - torch.from_numpy(g[k])).abs().max())
        print("%s %s: max-abs vs the reference %.3e" % (name, k, d))
        assert d <= 1e-3, (k, d)
    assert m.memories["frames"] == list(range(S - 1))               # every frame but the last was memorised, none evicted


# ------------------------------------------------------------------------------------------------ csrc/losses.hip, term by term
# Sums: 2e-6 relative to the float64 reference -- about four times the farthest the float32-element yardstick lies from it (3.6e-7 to
# 4.4e-7 with the seed, exclusion acc2 on the smallest shapes; tests/test_glue_train_cpu.py prints the table).  Down arrays: 1e-6 absolute (yardstick
# 2.5e-7).  Tensors written elementwise: the bits of the float32 torch statement.
SUM_TOL, DOWN_TOL = 2e-6, 1e-6


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    from otvm_amd import lib
    lib.load()
    return gpu_util


def _lib():
    from otvm_amd import lib as L
    return L, L.load()


def _acc(G, n):
    return torch.zeros(n, dtype=torch.float64, device=G.DEV)


def _check_sums(name, shape, got, want, tol=SUM_TOL):
    from tests.train_loss_ref import rel
    d = rel(got, want)
    print("train margin %-22s %-16s %.3e of %.0e relative" % (name, "x".join(map(str, shape)), d, tol))
    assert d <= tol, (name, shape, got, want)


def _stream_ids():
    from tests import glue_train_cases as K
    return dict(argvalues=K.STREAM, ids=K.ids(K.STREAM))


@pytest.mark.parametrize("B,S,H,W", **_stream_ids())
def test_fba_comp_five_sums_and_tensors(G, B, S, H, W):
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    x = K.loss_inputs(B, S, H, W)
    ref, f32 = LR.fba_comp(*x), LR.fba_comp(*x, dt=torch.float32)
    pred, gts, tm, fgs, bgs, imgs = (v.to(G.DEV).contiguous() for v in x)
    cF, cB, comp = (torch.full((B, S, 3, H, W), float("nan"), device=G.DEV) for _ in range(3))
    al = torch.full((B, S, 1, H, W), float("nan"), device=G.DEV)
    acc = _acc(G, 6)
    L.check(lib.otvm_loss_fba_comp(pred.data_ptr(), gts.data_ptr(), tm.data_ptr(), fgs.data_ptr(), bgs.data_ptr(), imgs.data_ptr(), B * S,
                                   H * W, cF.data_ptr(), cB.data_ptr(), comp.data_ptr(), al.data_ptr(), acc.data_ptr(), G.stream()))
    got = acc.cpu()
    assert float(got[5]) == 0.0
    for i, name in enumerate(("|a - gt|", "|cF gt + cB (1-gt) - img|", "|fg a + bg (1-a) - img|", "|cF - fg|", "|cB - bg|")):
        _check_sums("fba_comp " + name, (B, S, H, W), float(got[i]), ref["sums"][i])
    for name, t in (("alphas", al), ("Fs", cF), ("Bs", cB), ("comps", comp)):
        assert torch.equal(t.cpu(), f32[name]), name


@pytest.mark.parametrize("B,S,H,W", **_stream_ids())
def test_grad_l1_sum(G, B, S, H, W):
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    x, y = K.pair((B * S, H, W), seed=21)
    y[y < 0.3] = 0.0
    y[y > 0.8] = 1.0
    xd, yd, acc = x.to(G.DEV), y.to(G.DEV), _acc(G, 2)
    L.check(lib.otvm_loss_grad_l1(xd.data_ptr(), yd.data_ptr(), B * S, H, W, 1.001e-5, acc.data_ptr(), G.stream()))
    got = acc.cpu()
    assert float(got[1]) == 0.0
    _check_sums("grad_l1", (B, S, H, W), float(got[0]), LR.grad_l1(x, y))


@pytest.mark.parametrize("kind", ["scale8", "pm100"])
@pytest.mark.parametrize("B,S,H,W", **_stream_ids())
def test_ce3_sum_against_float64_cross_entropy(G, B, S, H, W, kind):
    L, lib = _lib()
    N = B * S
    g = torch.Generator().manual_seed(22)
    lg = torch.randn(N, 3, H, W, generator=g) * 8
    if kind == "pm100":
        lg = torch.where(lg > 0, torch.full_like(lg, 100.0), torch.full_like(lg, -100.0))
    cls = torch.randint(0, 3, (N, H, W), generator=g).to(torch.uint8)
    lgd, cd, acc = lg.to(G.DEV), cls.to(G.DEV), _acc(G, 2)
    L.check(lib.otvm_loss_ce3(lgd.data_ptr(), cd.data_ptr(), N, H * W, acc.data_ptr(), G.stream()))
    got = acc.cpu()
    want = float(F.cross_entropy(lg.double(), cls.long(), reduction="sum"))
    assert float(got[1]) == 0.0 and np.isfinite(float(got[0]))
    _check_sums("ce3 " + kind, (B, S, H, W), float(got[0]), want)


TEMPORAL = [(2, 3, 5, 7), (2, 4, 5, 7), (1, 2, 512, 544)]


@pytest.mark.parametrize("B,S,H,W", TEMPORAL, ids=["x".join(map(str, c)) for c in TEMPORAL])
def test_temporal_sum(G, B, S, H, W):
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    for Cn in (1, 3):
        x, y = K.pair((B, S, Cn, H, W), seed=23 + Cn)
        xd, yd, acc = x.to(G.DEV), y.to(G.DEV), _acc(G, 2)
        L.check(lib.otvm_loss_temporal(xd.data_ptr(), yd.data_ptr(), B, S, Cn * H * W, acc.data_ptr(), G.stream()))
        got = acc.cpu()
        assert float(got[1]) == 0.0
        _check_sums("temporal C=%d" % Cn, (B, S, H, W), float(got[0]), LR.temporal(x, y))


# A grid-stride loop is right with any grid: were lgrid to launch one block, every sum above would stay within its tolerance and only
# the time would change.  So the cap's other half -- that a crop above it still gets 2048 blocks -- is pinned as a rate.  One block is
# one of 256 compute units, which streams at most about 90 GB/s; the whole chip reaches about 6,300 GB/s.  The floor is 200 GB/s.
GRID_FLOOR_GBPS = 200.0


def test_fba_comp_above_the_cap_still_fills_the_chip(G):
    L, lib = _lib()
    B, S, H, W = 2, 4, 512, 544
    N, P = B * S, H * W
    g = torch.Generator(device=G.DEV).manual_seed(31)
    pred, gts, tm, fgs, bgs, imgs = (torch.rand(N, c, H, W, generator=g, device=G.DEV) for c in (7, 1, 1, 3, 3, 3))
    tm = (tm > 0.5).float()
    cF, cB, comp, al = (torch.empty(N, c, H, W, device=G.DEV) for c in (3, 3, 3, 1))
    acc = _acc(G, 5)
    nbytes = N * P * 4 * (7 + 1 + 1 + 9 + 10)                     # every input plane read once, ten planes written
    rate = G.best_gbps(lambda: L.check(lib.otvm_loss_fba_comp(pred.data_ptr(), gts.data_ptr(), tm.data_ptr(), fgs.data_ptr(), bgs.data_ptr(),
                                                              imgs.data_ptr(), N, P, cF.data_ptr(), cB.data_ptr(), comp.data_ptr(),
                                                              al.data_ptr(), acc.data_ptr(), G.stream())), nbytes)
    print("train margin fba_comp %dx%dx%dx%d: %.0f GB/s of its %.0f MB, floor %.0f GB/s" % (B, S, H, W, rate, nbytes / 1e6, GRID_FLOOR_GBPS))
    assert rate >= GRID_FLOOR_GBPS


def _excl_ids():
    from tests import glue_train_cases as K
    return dict(argvalues=K.EXCLUSION, ids=K.ids(K.EXCLUSION))


@pytest.mark.parametrize("B,S,H,W", **_excl_ids())
def test_exclusion_level_per_frame_and_per_image_sums(G, B, S, H, W):
    """acc1 per frame (over the batch), acc2 per (b, frame); W = 1 / H = 1 make one gradient identically zero, whose sums stay 0."""
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    i1, i2 = K.pair((B, S, 3, H, W), seed=11)
    w1, w2 = LR.exclusion_level(i1, i2)
    d1, d2 = i1.to(G.DEV), i2.to(G.DEV)
    acc = _acc(G, S * 4 + B * S * 2 + 2)
    L.check(lib.otvm_loss_exclusion_level(d1.data_ptr(), d2.data_ptr(), B, S, H, W, 1.001e-5, acc.data_ptr(),
                                          acc.data_ptr() + 8 * S * 4, G.stream()))
    got = acc.cpu()
    assert float(got[-1]) == 0.0 and float(got[-2]) == 0.0
    g1, g2 = got[:S * 4].reshape(S, 4), got[S * 4:-2].reshape(B * S, 2)
    if W == 1:
        assert not g1[:, [0, 2]].any() and not g2[:, 0].any() and not w1[:, [0, 2]].any()
    if H == 1:
        assert not g1[:, [1, 3]].any() and not g2[:, 1].any() and not w1[:, [1, 3]].any()
    _check_sums("exclusion acc1", (B, S, H, W), g1, w1)
    _check_sums("exclusion acc2", (B, S, H, W), g2, w2)


def _lap_ids():
    from tests import glue_train_cases as K
    return dict(argvalues=K.LAP, ids=K.ids(K.LAP))


@pytest.mark.parametrize("N,H,W", **_lap_ids())
def test_lap_level_sum_and_both_down_arrays(G, N, H, W):
    """Weights 1 and 16 into one accumulator (as _fba_loss adds its five levels up): 17 x the float64 sum; both down arrays within
    1e-6 of the float64 Gaussian reduction."""
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    ci, ct = K.pair((N, H, W), seed=12)
    s1, wi, wt = LR.lap_level(ci, ct, 1.0)
    cid, ctd, acc = ci.to(G.DEV), ct.to(G.DEV), _acc(G, 2)
    for weight, total in ((1.0, 1.0), (16.0, 17.0)):
        di, dt = (torch.full((N, H // 2, W // 2), float("nan"), device=G.DEV) for _ in range(2))
        L.check(lib.otvm_loss_lap_level(cid.data_ptr(), ctd.data_ptr(), N, H, W, weight, di.data_ptr(), dt.data_ptr(), acc.data_ptr(),
                                        G.stream()))
        got = acc.cpu()
        assert float(got[1]) == 0.0
        _check_sums("lap_level weight %g" % weight, (N, H, W), float(got[0]), total * s1)
        d = max(float((di.cpu().double() - wi).abs().max()), float((dt.cpu().double() - wt).abs().max()))
        print("train margin lap_level down arrays     %-16s %.3e of %.0e absolute" % ("x".join(map(str, (N, H, W))), d, DOWN_TOL))
        assert d <= DOWN_TOL


def _pool_ids():
    from tests import glue_train_cases as K
    return dict(argvalues=K.AVGPOOL, ids=K.ids(K.AVGPOOL))


@pytest.mark.parametrize("N,H,W", **_pool_ids())
def test_avgpool2_bits(G, N, H, W):
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    x, _ = K.pair((N, H, W), seed=13)
    xd = x.to(G.DEV)
    y = torch.full((N * (H // 2) * (W // 2) + 4,), float("nan"), device=G.DEV)
    L.check(lib.otvm_avgpool2(xd.data_ptr(), N, H, W, y.data_ptr(), G.stream()))
    got = y.cpu()
    assert torch.isnan(got[-4:]).all()
    assert torch.equal(got[:-4].reshape(N, H // 2, W // 2), LR.avgpool2(x, torch.float32))


@pytest.mark.parametrize("B,S,H,W", **_stream_ids())
def test_scale_flip_trimask_cls_vis_bits(G, B, S, H, W):
    L, lib = _lib()
    N, P = B * S, H * W
    g = torch.Generator().manual_seed(24)
    tri, gt = torch.rand(N, 3, H, W, generator=g), torch.rand(N, H, W, generator=g)
    tri[:, 1][tri[:, 0] > 0.9] = 0.95                            # ties between two classes: the first maximum wins
    tri[:, 0][tri[:, 0] > 0.9] = 0.95
    x = torch.rand(N, 3, H, W, generator=g) * 255
    tri_d, gt_d, x_d = tri.to(G.DEV), gt.to(G.DEV), x.to(G.DEV)
    mask, vis = (torch.full((N, H, W), float("nan"), device=G.DEV) for _ in range(2))
    cls = torch.full((N, H, W), 9, dtype=torch.uint8, device=G.DEV)
    y = torch.full((N, 3, H, W), float("nan"), device=G.DEV)
    L.check(lib.otvm_trimask(tri_d.data_ptr(), N, P, mask.data_ptr(), cls.data_ptr(), gt_d.data_ptr(), vis.data_ptr(), G.stream()))
    L.check(lib.otvm_scale_flip3(x_d.data_ptr(), N, P, 1.0 / 255, y.data_ptr(), G.stream()))
    want = tri.max(dim=1)[1]
    assert torch.equal(cls.cpu().long(), want) and torch.equal(mask.cpu(), (want == 1).float())
    assert torch.equal(vis.cpu(), torch.where(want == 1, torch.ones_like(gt) * 128 * (1. / 255), gt))
    assert torch.equal(y.cpu(), x.flip([1]) * (1.0 / 255))


def _loss_ids():
    from tests import glue_train_cases as K
    return dict(argvalues=K.FBA_LOSS, ids=K.ids(K.FBA_LOSS))


@pytest.mark.parametrize("B,S,H,W", **_loss_ids())
def test_fba_loss_end_to_end_against_the_float64_oracle(G, B, S, H, W):
    """_fba_loss's three sums within 2e-6 of train_oracle.fba_loss in float64: S = 1 (no temporal term) with B = 1, the existing
    test's shape, and a crop above every grid cap of csrc/losses.hip.  The returned tensors are the float32 statement's bits."""
    from oracle import train_oracle as T
    from otvm_amd.train import _fba_loss
    from tests import glue_train_cases as K, train_loss_ref as LR
    L, lib = _lib()
    x = K.loss_inputs(B, S, H, W)
    pred, gts, tm, fgs, bgs, imgs = x
    want = T.fba_loss(*(v.double() for v in (pred, tm, gts, fgs, bgs, imgs)))
    got = _fba_loss(lib, G.stream(), torch.device(G.DEV), *(v.to(G.DEV).contiguous() for v in x), B, S, H, W)
    for i, name in enumerate(("L_alpha_comp", "L_lap", "L_grad")):
        _check_sums("_fba_loss " + name, (B, S, H, W), got[i], float(want[i]))
    f32 = LR.fba_comp(*x, dt=torch.float32)
    for i, name in ((3, "alphas"), (4, "comps"), (5, "Fs"), (6, "Bs")):
        assert torch.equal(got[i].cpu(), f32[name]), name


def test_loss_entries_refuse_bad_sizes(G):
    """Odd or too small sizes for the pyramid levels, one frame for the temporal term, more images than the grid's y extent: non-zero
    before anything is launched (the output buffers keep their canaries)."""
    L, lib = _lib()
    x = torch.rand(3 * 65550 + 4096, device=G.DEV)              # sized so that even a call that went through would stay in bounds
    out = torch.full((4096,), float("nan"), device=G.DEV)
    acc = _acc(G, 4370 * 4 + 5 * 4370 * 2)
    p, o, a, st = x.data_ptr(), out.data_ptr(), acc.data_ptr(), G.stream()
    for H, W in ((5, 4), (4, 5), (2, 4), (4, 2)):
        assert lib.otvm_loss_lap_level(p, p, 1, H, W, 1.0, o, o + 2048, a, st) != 0, (H, W)
    assert lib.otvm_avgpool2(p, 1, 3, 4, o, st) != 0 and lib.otvm_avgpool2(p, 1, 4, 3, o, st) != 0
    assert lib.otvm_loss_temporal(p, p, 1, 1, 16, a, st) != 0
    assert lib.otvm_loss_exclusion_level(p, p, 5, 4370, 1, 1, 1.001e-5, a, a + 8 * 4370 * 4, st) != 0        # 5 * 4370 * 3 = 65,550 images
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and not acc.cpu().any()
