"""The restatements behind tests/test_gpu_glue.py and the new tests of tests/test_gpu_train.py, held to definitions on the CPU (no
GPU): tests/glue_ref.py against the oracle's statements and F.interpolate, tests/train_loss_ref.py against train_oracle.fba_loss,
and the yardstick -- how far float32 elements with float64 sums lie from float64 throughout -- printed per term."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_oracle as T
from tests import glue_ref as R
from tests import glue_train_cases as K
from tests import train_loss_ref as LR

f64 = torch.float64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------ glue
@pytest.mark.parametrize("h4,w4", [c[:2] for c in K.UPSAMPLE[:5]], ids=K.ids([c[:2] for c in K.UPSAMPLE[:5]]))
def test_restated_upsample_is_bilinear_x4(h4, w4):
    """Within 2^-22 max(1, max|ref|) of F.interpolate in float64: three roundings of at most half an ulp of the largest value."""
    for scale in (1.0, 8.0, 30.0):
        lg = K.logits(h4, w4, scale, seed=h4 * 100 + w4)
        got = R.upsample4_logits(lg)
        want = F.interpolate(torch.from_numpy(lg).to(f64)[None], scale_factor=4, mode="bilinear", align_corners=False)[0].numpy()
        assert got.shape == want.shape == (3, 4 * h4, 4 * w4) and got.dtype == np.float32
        top = max(1.0, float(np.abs(want).max()))
        d = float(np.abs(got.astype(np.float64) - want).max())
        print("upsample4 restatement %dx%d scale %g: %.3e of the largest value" % (h4, w4, scale, d / top))
        assert d <= 2.0 ** -22 * top


@pytest.mark.parametrize("H,W,Hp,Wp,lh,lw", K.PREPROCESS[:3], ids=K.ids(K.PREPROCESS[:3]))
def test_restated_preprocess_is_the_oracles_statements(H, W, Hp, Wp, lh, lw):
    """oracle/otvm_oracle.py, frame: flip, * 1/255, composite, F.pad, (img - mean) / std -- bit for bit in float32, for the three
    input routes and the three mean / std sets."""
    assert np.float32(1) / np.float32(255) == np.float32(1.0 / 255)
    a, fg, bg = K.preprocess_inputs(H, W, seed=H + W)
    fg4, bg4 = (torch.from_numpy(K.planes_f32(x))[None] for x in (fg, bg))          # [1,3,H,W] BGR 0..255, as frame() takes them
    a4 = torch.from_numpy(a)[None, None]
    s = 1.0 / 255
    img = (fg4.flip([1]) * s) * a4 + (bg4.flip([1]) * s) * (1.0 - a4)
    imgp = F.pad(img, (lw, Wp - W - lw, lh, Hp - H - lh))
    routes = (dict(fg=K.planes_f32(fg), bg=K.planes_f32(bg)), dict(fg_u8=fg, bg_u8=bg, u8_rgb=False),
              dict(fg_u8=fg[..., ::-1].copy(), bg_u8=bg[..., ::-1].copy(), u8_rgb=True))
    for src in routes:
        r = R.preprocess(a, Hp, Wp, lh, lw, **src)
        assert np.array_equal(bits(r["scaled_imgs"]), bits(img[0].numpy()))
        assert np.array_equal(bits(r["imgp"]), bits(imgp[0].numpy()))
        for name, mk, sk in (("n", "mean", "std"), ("q", "mean_q", "std_q"), ("m", "mean_m", "std_m")):
            mean, std = (torch.tensor(R.NORMS[k], dtype=torch.float32).reshape(1, 3, 1, 1) for k in (mk, sk))
            assert np.array_equal(bits(r[name]), bits(((imgp - mean) / std)[0].numpy())), name
    lanes = R.preprocess_lanes(r)
    assert lanes["x11"].shape == (Hp * Wp, 4) and lanes["d80"].shape == (Hp * Wp, 6) and not lanes["x11"][:, 3].any()
    assert np.array_equal(lanes["d80"][:, 3:].T.reshape(3, Hp, Wp), r["imgp"])
    # a wrong channel order is visible in these inputs
    wrong = R.preprocess(a, Hp, Wp, lh, lw, fg_u8=fg, bg_u8=bg, u8_rgb=True)
    assert not np.array_equal(wrong["scaled_imgs"], r["scaled_imgs"])


def test_restated_trimap_to_sm():
    tri = np.arange(3 * 5, dtype=np.float32).reshape(3, 5)
    sm = np.full((5, 8), np.nan, np.float32)
    out = R.trimap_to_sm(tri, sm)
    assert np.array_equal(out[:, 3], tri[1]) and np.array_equal(out[:, 4], tri[2])
    assert np.isnan(out[:, [0, 1, 2, 5, 6, 7]]).all() and np.isnan(sm).all()


# ------------------------------------------------------------------------------------------------ loss terms
@pytest.mark.parametrize("B,S,H,W", [(2, 3, 64, 96), (1, 1, 64, 64), (1, 2, 64, 64)], ids=K.ids([(2, 3, 64, 96), (1, 1, 64, 64), (1, 2, 64, 64)]))
def test_float64_terms_reassemble_to_the_oracles_loss(B, S, H, W):
    """The per-term split, put together with _fba_loss's weights, is train_oracle.fba_loss (float64, 1e-12 relative)."""
    x = [v.to(f64) for v in K.loss_inputs(B, S, H, W)]
    pred, gts, tm, fgs, bgs, imgs = x
    want = T.fba_loss(pred, tm, gts, fgs, bgs, imgs)
    t = LR.all_terms(*x, dt=f64)
    got = LR.loss_from_terms(t, B, S, H, W)
    for name, g, w in zip(("L_alpha_comp", "L_lap", "L_grad"), got, want):
        assert abs(g - float(w)) <= 1e-12 * abs(float(w)), (name, g, float(w))
    for name, i in (("alphas", 3), ("comps", 4), ("Fs", 5), ("Bs", 6)):
        assert torch.equal(t[name], want[i]), name


def test_term_definitions_on_hand_cases():
    """avgpool2 is F.avg_pool2d; grad_l1 is l1_grad x count; ce3 is F.cross_entropy x count; one down array is the pyramid's."""
    x, y = K.pair((3, 6, 10), seed=5)
    for dt in (f64, torch.float32):
        assert torch.equal(LR.avgpool2(x, dt), F.avg_pool2d(x.to(dt)[:, None], 2, 2)[:, 0])
    assert abs(LR.grad_l1(x, y) - float(T.l1_grad(x.to(f64)[:, None], y.to(f64)[:, None])) * x.numel()) <= 1e-12
    lg, cls = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(1)) * 8, torch.randint(0, 3, (2, 5, 7))
    assert abs(LR.ce3(lg, cls) - float(F.cross_entropy(lg.to(f64), cls)) * cls.numel()) <= 1e-10
    a, b = K.pair((2, 8, 12), seed=6)
    s, da, db = LR.lap_level(a, b, 16.0)
    k = T.GAUSS.to(f64)[None, None]
    assert torch.equal(da, T._conv_gauss(a.to(f64)[:, None], k)[:, 0, ::2, ::2]) and da.shape == (2, 4, 6)
    pa, pb = T.laplacian_pyramid(a.to(f64)[:, None], 1), T.laplacian_pyramid(b.to(f64)[:, None], 1)
    assert abs(s - 16.0 * float((pa[0] - pb[0]).abs().sum())) <= 1e-12 * s
    # the exclusion statistics are per frame (acc1) and per (b, frame) (acc2): swapping two frames of one clip moves them
    i1, i2 = K.pair((2, 3, 3, 5, 7), seed=7)
    a1, a2 = LR.exclusion_level(i1, i2)
    p = [1, 0, 2]
    b1, b2 = LR.exclusion_level(i1[:, p], i2[:, p])
    assert torch.allclose(b1, a1[p], rtol=1e-14) and torch.allclose(b2.reshape(2, 3, 2), a2.reshape(2, 3, 2)[:, p], rtol=1e-14)
    assert not torch.allclose(a1[0], a1[1], rtol=1e-3)


def test_yardstick_float32_elements_against_float64(capsys):
    """Prints how far form (b) (float32 elements, float64 sums) lies from form (a) (float64) per term, at the shapes the GPU tests
    use; the GPU tests' 2e-6 (sums) and 1e-6 (down arrays) are about four times the largest figure."""
    rows = []
    for B, S, H, W in K.STREAM:
        x = K.loss_inputs(B, S, H, W)
        a, b = LR.fba_comp(*x, dt=f64), LR.fba_comp(*x, dt=torch.float32)
        rows.append(("fba_comp sums", (B, S, H, W), LR.rel(b["sums"], a["sums"])))
        al, gt = x[0][:, :, 0].reshape(-1, H, W), x[1].reshape(-1, H, W)
        rows.append(("grad_l1", (B, S, H, W), LR.rel(LR.grad_l1(al, gt, torch.float32), LR.grad_l1(al, gt))))
        if S > 1:
            rows.append(("temporal", (B, S, H, W), LR.rel(LR.temporal(x[3], x[4], torch.float32), LR.temporal(x[3], x[4]))))
        lg = torch.randn(B * S, 3, H, W, generator=torch.Generator().manual_seed(9)) * 8
        cls = torch.randint(0, 3, (B * S, H, W), generator=torch.Generator().manual_seed(10))
        rows.append(("ce3", (B, S, H, W), LR.rel(LR.ce3(lg, cls, torch.float32), LR.ce3(lg, cls))))
    for B, S, H, W in K.EXCLUSION:
        i1, i2 = K.pair((B, S, 3, H, W), seed=11)
        a, b = LR.exclusion_level(i1, i2), LR.exclusion_level(i1, i2, torch.float32)
        rows.append(("exclusion acc1", (B, S, H, W), LR.rel(b[0], a[0])))
        rows.append(("exclusion acc2", (B, S, H, W), LR.rel(b[1], a[1])))
    down = []
    for N, H, W in K.LAP:
        ci, ct = K.pair((N, H, W), seed=12)
        a, b = LR.lap_level(ci, ct, 16.0), LR.lap_level(ci, ct, 16.0, torch.float32)
        rows.append(("lap_level sum", (N, H, W), LR.rel(b[0], a[0])))
        down.append(((N, H, W), max(float((b[k].to(f64) - a[k]).abs().max()) for k in (1, 2))))
    with capsys.disabled():
        for name, shape, d in rows:
            print("yardstick %-16s %-18s float32 elements vs float64: %.3e relative" % (name, "x".join(map(str, shape)), d))
        for shape, d in down:
            print("yardstick %-16s %-18s float32 elements vs float64: %.3e absolute" % ("lap down", "x".join(map(str, shape)), d))
    assert max(d for _, _, d in rows) <= 5e-7 and max(d for _, d in down) <= 2.5e-7

