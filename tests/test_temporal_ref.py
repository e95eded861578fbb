"""The numpy restatement of the temporal stabilisation (tests/temporal_ref.py) by itself, on the CPU: its closed forms, and the
property it exists for -- on synthetic clips with noise in the unknown band, the flow-compensated filter lowers dtSSD and SAD
against the ground truth by more than 10 %, and by more than the same filter without motion compensation does.

There is no trained checkpoint here: the filter is checked by definition and by property on synthetic clips, not by quality
on real footage."""
import numpy as np
import pytest

from tests import farneback_ref as FB
from tests import temporal_ref as R

F32 = np.float32


def _planes(seed, H, W):
    rng = np.random.default_rng(seed)
    a = rng.random((H, W)).astype(F32) * F32(1.4) - F32(0.2)               # (values outside [0,1] too)
    prev = rng.random((H, W)).astype(F32)
    g = rng.integers(0, 256, (H, W)).astype(np.uint8)
    gp = np.clip(g.astype(np.int32) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
    cls = rng.integers(0, 3, (H, W))
    tri = np.stack([cls == c for c in range(3)]).astype(F32)
    return a, prev, g, gp, tri


def test_luma_is_the_integer_formula():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    want = np.array([[(int(p[0]) * 1868 + int(p[1]) * 9617 + int(p[2]) * 4899 + 8192) >> 14 for p in row] for row in img], np.uint8)
    assert np.array_equal(R.luma_u8(img), want)
    assert np.array_equal(R.luma_u8(img[..., ::-1], rgb=True), want)
    assert R.luma_u8(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255 and R.luma_u8(np.zeros((1, 1, 3), np.uint8))[0, 0] == 0


def test_strength_zero_returns_the_clamped_input():
    a, prev, g, gp, tri = _planes(1, 23, 31)
    flow = np.random.default_rng(2).normal(0, 3, (23, 31, 2)).astype(F32)
    for t in (None, tri):
        out, u8 = R.blend(a, prev, g, gp, flow, t, strength=0.0)
        assert np.array_equal(out.view(np.uint32), np.clip(a, 0, 1).view(np.uint32))
        assert np.array_equal(u8, np.trunc(np.clip(a, 0, 1) * F32(255)).astype(np.uint8))
    out, u8 = R.first(a)
    assert np.array_equal(out.view(np.uint32), np.clip(a, 0, 1).view(np.uint32))


def test_zero_flow_is_the_closed_form():
    a, prev, g, gp, tri = _planes(3, 19, 27)
    k, itc, ita = F32(0.5), F32(1) / F32(24), F32(1) / F32(0.5)
    wc = np.maximum(F32(0), F32(1) - np.abs(g.astype(F32) - gp.astype(F32)) * itc)
    wa = np.maximum(F32(0), F32(1) - np.abs(a - prev) * ita)
    for t, gate in ((None, np.ones_like(a)), (tri, tri[1])):
        want = np.clip(a + (((k * wc) * wa) * gate) * (prev - a), 0, 1).astype(F32)
        out, u8 = R.blend(a, prev, g, gp, np.zeros((19, 27, 2), F32), t)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(u8, np.trunc(want * F32(255)).astype(np.uint8))
    assert np.array_equal(out[tri[1] == 0], np.clip(a, 0, 1)[tri[1] == 0])       # outside the unknown class: untouched


def test_integer_flow_samples_the_shifted_plane():
    a, prev, g, gp, _ = _planes(4, 21, 33)
    H, W = a.shape
    for dx, dy in ((2, 1), (-3, 2), (0, -4)):
        flow = np.zeros((H, W, 2), F32)
        flow[..., 0], flow[..., 1] = dx, dy
        sx = (np.arange(W, dtype=F32)[None, :] + flow[..., 0])
        sy = (np.arange(H, dtype=F32)[:, None] + flow[..., 1])
        ok = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        s = R.sample(prev, sx, sy, ok)
        ys, xs = np.nonzero(ok)
        assert np.array_equal(s[ys, xs], prev[ys + dy, xs + dx]) and ok.any() and not ok.all()
        assert not s[~ok].any()
        # where the target leaves the frame the alpha passes through
        out, _ = R.blend(a, prev, g, gp, flow, strength=1.0)
        assert np.array_equal(out[~ok], np.clip(a, 0, 1)[~ok])


def test_gate_is_first_max_argmax_and_nan_closes_it():
    tri = np.array([[[0.2, 0.5, 0.5, np.nan, 0.1]], [[0.5, 0.5, 0.3, 0.9, np.nan]], [[0.5, 0.1, 0.5, 0.1, 0.2]]], F32)
    assert R.gate_of(tri, 1, 5, 1).tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0]]
    assert R.gate_of(tri, 2, 9, 2).tolist() == [[1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 2       # clamped at the edge


def test_non_finite_alpha_passes_through_with_byte_zero():
    a, prev, g, gp, _ = _planes(5, 6, 9)
    a[1, 2], a[3, 4], a[5, 8] = np.nan, np.inf, -np.inf
    out, u8 = R.blend(a, prev, g, gp, np.zeros((6, 9, 2), F32))
    bad = ~np.isfinite(a)
    assert np.array_equal(out.view(np.uint32)[bad], a.view(np.uint32)[bad]) and not u8[bad].any()
    assert np.isfinite(out[~bad]).all()


@pytest.mark.parametrize("idx", range(len(R.CLIPS)))
def test_flow_compensation_lowers_dtssd_and_sad(idx):
    c = R.clip_case(idx)
    stab, _ = R.chain(c["frames"], c["raws"], c["flows"], c["tris"])
    H, W = c["raws"][0].shape
    zero, _ = R.chain(c["frames"], c["raws"], [np.zeros((H, W, 2), F32)] * R.T_CLIP, c["tris"])
    dt, sd = R.ratios(stab, c["raws"], c["gts"])
    dt0, sd0 = R.ratios(zero, c["raws"], c["gts"])
    print("clip %s: dtSSD ratio %.3f (zero flow %.3f)  SAD ratio %.3f (zero flow %.3f)" % (R.CLIPS[idx], dt, dt0, sd, sd0))
    assert dt <= 0.9 and sd <= 0.9
    assert dt < dt0 and sd < sd0


def test_negated_flow_does_not_pass():
    """The control that tells the flow's direction: with the flow negated the first clip stays above 0.9."""
    c = R.clip_case(0)
    neg, _ = R.chain(c["frames"], c["raws"], [None] + [-f for f in c["flows"][1:]], c["tris"])
    dt, sd = R.ratios(neg, c["raws"], c["gts"])
    print("negated flow: dtSSD ratio %.3f  SAD ratio %.3f" % (dt, sd))
    assert dt > 0.9 and sd > 0.9


@pytest.mark.parametrize("idx", range(len(R.CLIPS)))
def test_flow_of_a_translation_is_minus_v(idx):
    H, W, v, seed = R.CLIPS[idx]
    fr = R.translated(H, W, 2, v, seed)
    flow = FB.farneback(R.luma_u8(fr[1]), R.luma_u8(fr[0]), np.float32)
    med = np.median(flow[8:-8, 8:-8].reshape(-1, 2), 0)
    print("v %s: interior median flow %s" % (v, med))
    assert abs(med[0] + v[0]) <= 0.5 and abs(med[1] + v[1]) <= 0.5
