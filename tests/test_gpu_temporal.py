"""Temporal stabilisation of alpha on the device (otvm_luma_u8 / otvm_temporal_blend, csrc/temporal.hip) against the numpy
restatement (tests/temporal_ref.py), bit for bit, and the layers above it: temporal.TemporalStabiliser,
run_video_matte(stabilise=...), eval_cli --stabilise.

There is no trained checkpoint here: the filter is checked by definition and by property on synthetic clips, not by quality on
real footage.

Against the all-numpy chain on the float64 flow the stabiliser's bound is max|gpu - f64| <= max(3 max|f32 - f64|, 1e-6) per clip,
f32 / f64 being the restatement's chain on the restated float32 / float64 flows: the device's flow is a second float32
evaluation, so its distance to f64 is of the size of f32's (the rule of tests/test_gpu_messddt.py).  The margins measured on an
MI355X are in profiles/temporal_margins.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import temporal_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"


def _lib():
    from otvm_amd import lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_luma(img, rgb, offset=0):
    """otvm_luma_u8 through the C ABI; offset > 0 puts both bases ``offset`` bytes past an aligned address."""
    L, lib = _lib()
    H, W = img.shape[:2]
    src = torch.zeros(H * W * 3 + offset, dtype=torch.uint8, device=DEV)
    src[offset:] = dev(img).reshape(-1)
    out = torch.full((H * W + offset + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    L.check(lib.otvm_luma_u8(src.data_ptr() + offset, H, W, int(rgb), out.data_ptr() + offset, _stream()), "luma_u8")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:offset] == 0xA5).all() and (o[offset + H * W:] == 0xA5).all()            # nothing written outside the plane
    return o[offset:offset + H * W].reshape(H, W)


def device_blend(alpha, prev, grey, grey_prev, flow, tri=None, tri_scale=1, strength=0.5, tau_colour=24.0, tau_alpha=0.5,
                 want_u8=True):
    L, lib = _lib()
    H, W = alpha.shape
    d = [dev(x) for x in (alpha, prev, grey, grey_prev, flow, tri)]
    out = torch.full((H * W + 4,), -7.0, dtype=torch.float32, device=DEV)
    u8 = torch.full((H * W + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    p = L.TemporalParams()
    p.H, p.W = H, W
    p.alpha, p.prev, p.grey, p.grey_prev, p.flow, p.tri = [None if x is None else x.data_ptr() for x in d]
    if tri is not None:
        p.th, p.tw, p.tri_scale = tri.shape[1], tri.shape[2], tri_scale
    p.strength = strength
    p.inv_tau_colour, p.inv_tau_alpha = float(F32(1) / F32(tau_colour)), float(F32(1) / F32(tau_alpha))
    p.out, p.out_u8 = out.data_ptr(), u8.data_ptr() if want_u8 else None
    L.check(lib.otvm_temporal_blend(C.byref(p), _stream()), "temporal_blend")
    torch.cuda.synchronize()
    o, b = out.cpu().numpy(), u8.cpu().numpy()
    assert (o[H * W:] == -7.0).all() and (b[H * W:] == 0xA5).all()                      # nothing written past the planes
    assert want_u8 or (b == 0xA5).all()
    return o[:H * W].reshape(H, W), b[:H * W].reshape(H, W)


def blend_inputs(seed, H, W, tri_scale=None):
    """Random planes with the planted cases: the flow N(0, 3) with NaN, +-inf, -0.0, integers, targets exactly at W-1 / H-1 and
    1e-6 outside the frame; alpha with values outside [0,1], -0.0 and non-finite ones; a trimap with ties and NaN."""
    rng = np.random.default_rng(seed)
    N = H * W
    alpha = (rng.random((H, W)) * 1.4 - 0.2).astype(F32)
    prev = rng.random((H, W)).astype(F32)
    prev.reshape(-1)[rng.permutation(N)[:max(1, N // 16)]] = 0.0
    prev.reshape(-1)[rng.permutation(N)[:max(1, N // 16)]] = 1.0
    grey = rng.integers(0, 256, (H, W)).astype(np.uint8)
    gp = np.clip(grey.astype(np.int32) + np.rint(rng.normal(0, 10, (H, W))).astype(np.int32), 0, 255).astype(np.uint8)
    gp = np.roll(gp, (1, -2), (0, 1))
    flow = rng.normal(0, 3, (H, W, 2)).astype(F32)
    ys, xs = np.unravel_index(rng.permutation(N), (H, W))
    plants = [lambda x, y: (np.nan, 0.5), lambda x, y: (0.5, np.nan), lambda x, y: (np.inf, 0.0), lambda x, y: (0.0, -np.inf),
              lambda x, y: (-0.0, -0.0), lambda x, y: (-0.0, 1.0), lambda x, y: (2.0, -1.0), lambda x, y: (-1.0, 3.0),
              lambda x, y: (W - 1 - x, 0.25), lambda x, y: (0.25, H - 1 - y), lambda x, y: (W - 1 - x, H - 1 - y),
              lambda x, y: (-x, -y), lambda x, y: (-x - 1e-6, 0.0), lambda x, y: (0.0, -y - 1e-6),
              lambda x, y: (W - 1 - x + 1e-6, 0.0), lambda x, y: (0.0, H - 1 - y + 1e-6), lambda x, y: (1e30, -1e30)]
    for i in range(min(N, 4 * len(plants)) if N >= len(plants) else len(plants)):
        x, y = int(xs[i % N]), int(ys[i % N])
        flow[y, x] = plants[i % len(plants)](x, y)
    # pixels of the first column / row whose target lies 1e-6 outside (there -x - 1e-6 is not rounded away)
    flow[H // 2, 0] = (-1e-6, 0.0)
    flow[0, W // 2] = (0.0, -1e-6)
    for i, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 3e38, -3e38)):
        alpha.reshape(-1)[(7 * i + 3) % N] = v
    tri = None
    if tri_scale is not None:
        th, tw = -(-H // tri_scale), -(-W // tri_scale)
        tri = (rng.integers(0, 5, (3, th, tw)) * 0.25).astype(F32)                       # quantised: ties of every kind
        tri.reshape(-1)[rng.permutation(3 * th * tw)[:max(1, th * tw // 8)]] = np.nan
    return alpha, prev, grey, gp, flow, tri


# (5, 2): every pair of taps starts at column 0; (9, 8): two whole 16-byte groups per row and a trimap read as vectors
SHAPES = [(1, 1), (1, 7), (3, 5), (37, 53), (130, 257), (64, 96), (5, 2), (9, 8)]


@pytest.mark.parametrize("H,W", SHAPES[:5], ids=["%dx%d" % s for s in SHAPES[:5]])
def test_luma_bit_identical(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    img.reshape(-1, 3)[0] = 255
    for rgb in (False, True):
        want = R.luma_u8(img, rgb)
        assert np.array_equal(device_luma(img, rgb), want), rgb
        assert np.array_equal(device_luma(img, rgb, offset=1), want), rgb               # unaligned bases: pixel by pixel


def _check_blend(H, W, seed):
    for tri_scale in (None, 1, 3):
        a, prev, g, gp, flow, tri = blend_inputs(seed + (tri_scale or 0), H, W, tri_scale)
        for k in (0.5, 0.0, 1.0):
            want, want_u8 = R.blend(a, prev, g, gp, flow, tri, tri_scale or 1, strength=k)
            got, got_u8 = device_blend(a, prev, g, gp, flow, tri, tri_scale or 1, strength=k)
            assert np.array_equal(_bits(got), _bits(want)), (tri_scale, k, int((_bits(got) != _bits(want)).sum()))
            assert np.array_equal(got_u8, want_u8), (tri_scale, k)
        again, again_u8 = device_blend(a, prev, g, gp, flow, tri, tri_scale or 1, strength=1.0)
        assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(again_u8, got_u8)      # two calls, equal bits
        assert np.array_equal(_bits(device_blend(a, prev, g, gp, flow, tri, tri_scale or 1, strength=1.0, want_u8=False)[0]),
                              _bits(got))
        fin = np.isfinite(a)
        assert np.array_equal(_bits(got)[~fin], _bits(a)[~fin]) and not got_u8[~fin].any()
        assert got[fin].min() >= 0.0 and got[fin].max() <= 1.0
    # strength 0 is the clamped input, with any flow; so is the first frame (no previous alpha)
    got, got_u8 = device_blend(a, prev, g, gp, flow, strength=0.0)
    first, first_u8 = device_blend(a, None, None, None, None)
    want, want_u8 = R.first(a)
    for o, b in ((got, got_u8), (first, first_u8)):
        assert np.array_equal(_bits(o), _bits(want)) and np.array_equal(b, want_u8)
    assert np.array_equal(want[fin], np.clip(a, 0, 1)[fin])


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_blend_bit_identical(H, W):
    _check_blend(H, W, H * 131 + W)


def test_blend_bit_identical_1080p_every_element():
    H, W = 1080, 1920
    for tri_scale in (3, 1):
        a, prev, g, gp, flow, tri = blend_inputs(5, H, W, tri_scale)
        want, want_u8 = R.blend(a, prev, g, gp, flow, tri, tri_scale)
        got, got_u8 = device_blend(a, prev, g, gp, flow, tri, tri_scale)
        assert np.array_equal(_bits(got), _bits(want)), (tri_scale, int((_bits(got) != _bits(want)).sum()))
        assert np.array_equal(got_u8, want_u8), tri_scale
        fin = np.isfinite(a)
        assert float((got[fin] != np.clip(a[fin], 0, 1)).mean()) > 0.01                              # the filter acts


def test_blend_refuses_bad_arguments_and_launches_nothing():
    L, lib = _lib()
    H, W = 6, 8
    a, prev, g, gp, flow, tri = [dev(x) for x in blend_inputs(1, H, W, 1)]
    out = torch.full((H, W), -7.0, device=DEV)

    def params(**kw):
        p = L.TemporalParams()
        p.H, p.W, p.alpha, p.prev, p.grey, p.grey_prev, p.flow = H, W, a.data_ptr(), prev.data_ptr(), g.data_ptr(), gp.data_ptr(), flow.data_ptr()
        p.strength, p.inv_tau_colour, p.inv_tau_alpha, p.out = 0.5, 1 / 24.0, 2.0, out.data_ptr()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    assert lib.otvm_temporal_blend(C.byref(params()), _stream()) == 0
    torch.cuda.synchronize()
    out.fill_(-7.0)
    bad = [dict(H=0), dict(W=0), dict(H=65536), dict(alpha=None), dict(out=None), dict(out=prev.data_ptr()), dict(grey=None),
           dict(grey_prev=None), dict(flow=None), dict(strength=-0.1), dict(strength=1.5), dict(strength=float("nan")),
           dict(inv_tau_colour=0.0), dict(inv_tau_alpha=-1.0), dict(inv_tau_alpha=float("inf")),
           dict(tri=tri.data_ptr(), th=0, tw=W, tri_scale=1), dict(tri=tri.data_ptr(), th=H, tw=W, tri_scale=0),
           dict(alpha=a.data_ptr() + 2)]
    for change in bad:
        rc = lib.otvm_temporal_blend(C.byref(params(**change)), _stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.otvm_last_error().decode().startswith("otvm_temporal_blend"), change
        assert bool((out == -7.0).all()), change
    assert lib.otvm_temporal_blend(None, _stream()) != 0
    grey = torch.full((H, W), 0xA5, dtype=torch.uint8, device=DEV)
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    for args in ((None, H, W, 0, grey.data_ptr()), (img.data_ptr(), H, W, 0, None), (img.data_ptr(), 0, W, 0, grey.data_ptr()),
                 (img.data_ptr(), H, 0, 0, grey.data_ptr()), (img.data_ptr(), 65536, W, 0, grey.data_ptr())):
        assert lib.otvm_luma_u8(*args, _stream()) != 0 and lib.otvm_last_error().decode().startswith("otvm_luma_u8"), args
    torch.cuda.synchronize()
    assert bool((grey == 0xA5).all())


# ------------------------------------------------------------------------------------------------ TemporalStabiliser
def _run_stabiliser(c, **kw):
    """The device chain over clip ``c``: (outs [T,H,W], bytes, the flows of the steps (entry 0 None))"""
    from otvm_amd.temporal import TemporalStabiliser
    H, W = c["raws"][0].shape
    st = TemporalStabiliser(DEV, H, W, **kw)
    outs, u8s, flows = [], [], []
    for t in range(len(c["frames"])):
        o, b = st.step(dev(c["frames"][t]), dev(c["raws"][t]), trimap=dev(c["tris"][t]))
        assert (st.last_flow is None) == (t == 0)
        outs.append(o), u8s.append(b), flows.append(None if t == 0 else st.last_flow.clone())
    torch.cuda.synchronize()
    return (np.stack([o.cpu().numpy() for o in outs]), np.stack([b.cpu().numpy() for b in u8s]),
            [None if f is None else f.cpu().numpy() for f in flows], st)


@pytest.mark.parametrize("idx", range(len(R.CLIPS)))
def test_stabiliser_on_the_synthetic_clips(idx):
    c32, c64 = R.clip_case(idx, np.float32), R.clip_case(idx, np.float64)
    gpu, gpu_u8, flows, st = _run_stabiliser(c32)
    # fed the device's own flow, the restatement equals the device bit for bit at every step
    want, want_u8 = R.chain(c32["frames"], c32["raws"], flows, c32["tris"])
    assert np.array_equal(_bits(gpu), _bits(want)), [int((_bits(gpu[t]) != _bits(want[t])).sum()) for t in range(len(gpu))]
    assert np.array_equal(gpu_u8, want_u8)
    # against the all-numpy chain on the float64 flow
    f32, _ = R.chain(c32["frames"], c32["raws"], c32["flows"], c32["tris"])
    f64, _ = R.chain(c64["frames"], c64["raws"], c64["flows"], c64["tris"])
    ref_err = float(np.abs(f32.astype(np.float64) - f64).max())
    err = float(np.abs(gpu.astype(np.float64) - f64).max())
    flow_err = max(float(np.abs(flows[t].astype(np.float64) - c64["flows"][t]).max()) for t in range(1, len(flows)))
    flow_ref = max(float(np.abs(c32["flows"][t].astype(np.float64) - c64["flows"][t]).max()) for t in range(1, len(flows)))
    bound = max(3 * ref_err, 1e-6)
    print("clip %s: max|gpu-f64| %.3e  bound %.3e  max|f32-f64| %.3e  flow: max|gpu-f64| %.3e  max|f32-f64| %.3e"
          % (R.CLIPS[idx], err, bound, ref_err, flow_err, flow_ref))
    # the property, on the device's output
    H, W = c32["raws"][0].shape
    zero, _ = R.chain(c32["frames"], c32["raws"], [np.zeros((H, W, 2), F32)] * R.T_CLIP, c32["tris"])
    dt, sd = R.ratios(gpu, c32["raws"], c32["gts"])
    dt0, sd0 = R.ratios(zero, c32["raws"], c32["gts"])
    print("clip %s: dtSSD ratio %.3f (zero flow %.3f)  SAD ratio %.3f (zero flow %.3f)" % (R.CLIPS[idx], dt, dt0, sd, sd0))
    assert err <= bound
    assert dt <= 0.9 and sd <= 0.9 and dt < dt0 and sd < sd0
    # reset(): the next step starts a clip -- the clamped input
    st.reset()
    a = (np.random.default_rng(idx).random((H, W)) * 1.4 - 0.2).astype(F32)
    o, b = st.step(dev(c32["frames"][0]), dev(a), trimap=dev(c32["tris"][0]))
    w, wb = R.first(a)
    assert st.last_flow is None and np.array_equal(_bits(o.cpu().numpy()), _bits(w)) and np.array_equal(b.cpu().numpy(), wb)


@pytest.mark.parametrize("idx", range(len(R.CLIPS)))
def test_stabiliser_flow_of_a_translation_is_minus_v(idx):
    from otvm_amd.temporal import TemporalStabiliser
    H, W, v, seed = R.CLIPS[idx]
    fr = R.translated(H, W, 2, v, seed)
    st = TemporalStabiliser(DEV, H, W, region="all")
    zeros = torch.zeros((H, W), device=DEV)
    for f in fr:
        st.step(dev(f), zeros)
    med = np.median(st.last_flow.cpu().numpy()[8:-8, 8:-8].reshape(-1, 2), 0)
    print("v %s: interior median of last_flow %s" % (v, med))
    assert abs(med[0] + v[0]) <= 0.5 and abs(med[1] + v[1]) <= 0.5


def test_stabiliser_refusals_and_options():
    from otvm_amd.temporal import TemporalStabiliser, options_of
    for kw in (dict(strength=-0.1), dict(strength=1.1), dict(strength=float("nan")), dict(tau_colour=0), dict(tau_alpha=-1),
               dict(tau_alpha=float("inf")), dict(region="band"), dict(strength="x")):
        with pytest.raises(ValueError, match="TemporalStabiliser"):
            TemporalStabiliser(DEV, 8, 12, **kw)
    for hw in ((0, 4), (4, 0), (65536, 4)):
        with pytest.raises(ValueError):
            TemporalStabiliser(DEV, *hw)
    st = TemporalStabiliser(DEV, 8, 12)
    f, a, t = torch.zeros((8, 12, 3), dtype=torch.uint8, device=DEV), torch.zeros((8, 12), device=DEV), torch.zeros((3, 8, 12), device=DEV)
    for args, kw in (((f[:7], a), dict(trimap=t)), ((f.float(), a), dict(trimap=t)), ((f, a[:, :11]), dict(trimap=t)),
                     ((f, a.double()), dict(trimap=t)), ((f, a), dict()), ((f, a), dict(trimap=t[:2])),
                     ((f, a), dict(trimap=t, tri_scale=2)), ((f, a), dict(trimap=t, tri_scale=0)), ((f.cpu(), a), dict(trimap=t)),
                     ((f, a), dict(trimap=t.cpu()))):
        with pytest.raises(ValueError, match="TemporalStabiliser"):
            st.step(*args, **kw)
    assert st.state is None                                                              # a refused step changes nothing
    st.step(f, a, trimap=torch.zeros((3, 3, 4), device=DEV), tri_scale=3)
    TemporalStabiliser(DEV, 8, 12, region="all").step(f, a)                              # region "all" takes no trimap
    assert options_of(None) is None and options_of(False) is None and options_of(True) == {}
    assert options_of(0.25) == {"strength": 0.25} and options_of({"tau_alpha": 0.3}) == {"tau_alpha": 0.3}
    for bad in (1.5, "on", {"strenght": 0.5}, {"tau_colour": 0}):
        with pytest.raises(ValueError):
            options_of(bad)


# ------------------------------------------------------------------------------------------------ run_video_matte, eval_cli
H_, W_, T_ = 100, 150, 4


def _clip_masks():
    """Frames of the synthetic clip, a soft mask per frame that follows its moving disc, and the first frame's trimap."""
    from otvm_amd.synth_data import synthetic_clip
    frames, tri = synthetic_clip(H_, W_, T_, seed=53)
    yy, xx = np.mgrid[0:H_, 0:W_]
    ms = []
    for t in range(T_):
        r = np.sqrt((yy - H_ / 2 - 0.5 * t) ** 2 + (xx - W_ / 2 - 1.0 * t) ** 2)
        ms.append(np.floor(np.clip((H_ / 3.5 - r) / 3.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8))
    return frames, ms, tri


@pytest.fixture(scope="module")
def route(synth_sd, tmp_path_factory):
    """One model for all route tests, in one process, with the kernel configurations fixed (no timing runs, and eval_cli's own
    model launches the same ones)."""
    from otvm_amd import engine
    from tests.test_gpu_frame import _fresh_model
    old, old_auto = os.environ.get("OTVM_TUNE_FILE"), engine.AUTOTUNE
    os.environ["OTVM_TUNE_FILE"] = os.path.join(str(tmp_path_factory.mktemp("tune")), "tune.json")
    engine.AUTOTUNE = False
    try:
        yield (_fresh_model(synth_sd, 12, "f16x3"),) + _clip_masks()
    finally:
        engine.AUTOTUNE = old_auto
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


def _hand_driven(res, frames, work_scale=1, rgb=False, **kw):
    """A TemporalStabiliser fed the run's alpha_raw, the frames and the run's trimaps"""
    from otvm_amd.temporal import TemporalStabiliser
    st = TemporalStabiliser(DEV, H_, W_, **kw)
    outs = [st.step(dev(frames[t]), res["alpha_raw"][t].to(DEV), trimap=res["trimap"][t].to(DEV), tri_scale=work_scale, rgb=rgb)
            for t in range(len(frames))]
    return torch.stack([o[0] for o in outs]).cpu(), torch.stack([o[1] for o in outs]).cpu()


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_run_video_matte_masks_route(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, _ = route
    seen = []
    gt = [np.where(x > 127, 255, 0).astype(np.uint8) for x in ms]
    got = run_video_matte(m, frames, masks=ms, stabilise=True, on_frame=lambda i, a, u8, out: seen.append((i, a, u8)), gt_alpha_u8=gt)
    plain = run_video_matte(m, frames, masks=ms, gt_alpha_u8=gt)
    assert "alpha_raw" not in plain and sorted(set(got) - set(plain)) == ["alpha_raw"]
    assert _eq(got["alpha_raw"], plain["alpha"]) and _eq(got["trimap"], plain["trimap"])
    a, u8 = _hand_driven(got, frames)
    assert _eq(got["alpha"], a) and _eq(got["alpha_u8"], u8)
    assert not torch.equal(got["alpha"], got["alpha_raw"])                               # the filter acts on this clip
    for i, al, b in seen:                                                                # on_frame and the metrics: stabilised
        assert _eq(al.cpu(), a[i]) and _eq(b.cpu(), u8[i])
    assert [s[0] for s in seen] == list(range(T_))
    assert got["metrics"]["frames"] == T_ and got["metrics"]["sad_per_frame"] != plain["metrics"]["sad_per_frame"]
    want_sad = [float(np.abs(u8[t].numpy().astype(np.int64) - gt[t].astype(np.int64)).sum()) / 255.0 / 1000.0 for t in range(T_)]
    assert np.allclose(got["metrics"]["sad_per_frame"], want_sad, rtol=1e-12, atol=0)


def test_run_video_matte_trimap_route_with_options(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tri = route
    opts = dict(strength=0.8, tau_colour=12.0, tau_alpha=0.25, region="all")
    got = run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, stabilise=opts)
    plain = run_video_matte(m, frames, trimap=tri, skip=2, max_num=3)
    assert "alpha_raw" not in plain and _eq(got["alpha_raw"], plain["alpha"]) and got["bank_frames"] == plain["bank_frames"]
    a, u8 = _hand_driven(got, frames, **opts)
    assert _eq(got["alpha"], a) and _eq(got["alpha_u8"], u8)
    half = run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, stabilise=0.5)                # a float is the strength
    a, u8 = _hand_driven(half, frames, strength=0.5)
    assert _eq(half["alpha"], a) and _eq(half["alpha_u8"], u8) and not torch.equal(half["alpha"], got["alpha"])
    # forward-only keyframes (a trimap on frame 0, a correction later) and the alphas flow (without backgrounds) run too
    lab = np.full((H_, W_), 255, np.uint8)
    lab[:10, :10] = 0
    kf = run_video_matte(m, frames, keyframes={0: tri, 2: lab}, skip=2, max_num=3, stabilise=True)
    assert [s[0] for s in kf["schedule"]] == list(range(T_))
    a, u8 = _hand_driven(kf, frames)
    assert _eq(kf["alpha"], a) and _eq(kf["alpha_u8"], u8)
    al = run_video_matte(m, frames, alphas=[x.astype(np.float32) / 255 for x in ms], skip=2, max_num=3, stabilise=True)
    a, u8 = _hand_driven(al, frames)
    assert _eq(al["alpha"], a) and _eq(al["alpha_u8"], u8)


def test_run_video_matte_work_scale_with_foreground_and_background(route):
    from tests import fgr_ref
    from otvm_amd.video import run_video_matte
    m, frames, ms, tri = route
    colour = (10, 200, 30)
    for kw, scale in ((dict(work_scale=2), 2), (dict(), 1)):
        fs = []
        core = m.module
        got = run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, stabilise=True, foreground=True, new_background=colour,
                              on_frame=lambda i, a, u8, out: fs.append(None if scale > 1 else core._engine.last_fgr.cpu().numpy()), **kw)
        plain = run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, foreground=True, new_background=colour, **kw)
        assert _eq(got["alpha_raw"], plain["alpha"]) and "alpha_raw" not in plain
        a, u8 = _hand_driven(got, frames, work_scale=scale)
        assert _eq(got["alpha"], a) and _eq(got["alpha_u8"], u8)
        assert torch.equal(got["fgr_u8"][..., 3], got["alpha_u8"])
        assert torch.equal(got["fgr_u8"][..., :3], plain["fgr_u8"][..., :3])                       # F is not filtered
        assert not torch.equal(got["comp_u8"], plain["comp_u8"])
        if scale == 1:
            for t in range(T_):                                                                     # the bytes, from the run's F
                _, rgba, comp = fgr_ref.fgr_outputs(got["alpha"][t].numpy(), fs[t], colour)
                assert np.array_equal(got["fgr_u8"][t].numpy(), rgba) and np.array_equal(got["comp_u8"][t].numpy(), comp), t
        else:
            # (the full-resolution F is no part of the result: the next test takes it from the working-resolution stage)
            assert got["work_size"] == (50, 75) and tuple(got["trimap"].shape) == (T_, 3, 50, 75)
            assert tuple(got["comp_u8"].shape) == (T_, H_, W_, 3)
    assert m.module.foreground is False


def test_work_scale_foreground_bytes_equal_the_restatement(route):
    """work_scale=2 with foreground: fgr_u8 / comp_u8 equal tests/fgr_ref.fgr_outputs of the stabilised alpha and the run's
    full-resolution F (taken from the run's own working-resolution stage)."""
    from tests import fgr_ref
    from otvm_amd import video
    m, frames, ms, tri = route
    kept = []
    real = video._WorkingResolution.foreground_bytes

    def spy(self, i, alpha, dev_):
        kept.append(self.fgr_full.cpu().numpy())
        return real(self, i, alpha, dev_)
    video._WorkingResolution.foreground_bytes = spy
    try:
        bg = np.random.default_rng(3).integers(0, 256, (H_, W_, 3)).astype(np.uint8)
        got = video.run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, stabilise=True, new_background=bg, work_scale=2)
    finally:
        video._WorkingResolution.foreground_bytes = real
    assert len(kept) == T_
    for t in range(T_):
        _, rgba, comp = fgr_ref.fgr_outputs(got["alpha"][t].numpy(), kept[t], bg)
        assert np.array_equal(got["fgr_u8"][t].numpy(), rgba) and np.array_equal(got["comp_u8"][t].numpy(), comp), t


def test_run_video_matte_refusals_come_before_any_frame(route):
    from otvm_amd.video import run_video_matte
    m, frames, ms, tri = route
    calls = []
    handle = m.module.register_forward_pre_hook(lambda mod, args: calls.append(1))

    class Uploads(list):
        """a frame source that counts what is taken from it"""
        taken = 0

        def __getitem__(self, i):
            Uploads.taken += 1
            return list.__getitem__(self, i)
    try:
        src = Uploads(list(frames))
        with pytest.raises(ValueError, match="float"):
            run_video_matte(m, [f.astype(np.float32) for f in frames], trimap=tri, stabilise=True)
        with pytest.raises(ValueError, match="backgrounds"):
            run_video_matte(m, src, alphas=[x.astype(np.float32) / 255 for x in ms], backgrounds=list(frames), stabilise=True)
        with pytest.raises(ValueError, match="natural order"):
            run_video_matte(m, src, keyframes={2: tri}, stabilise=True)
        with pytest.raises(ValueError, match="strength"):
            run_video_matte(m, src, trimap=tri, stabilise=1.5)
        with pytest.raises(ValueError, match="stabilise"):
            run_video_matte(m, src, trimap=tri, stabilise="yes")
        with pytest.raises(TypeError):
            from otvm_amd.video import run_video_matte_batch
            run_video_matte_batch(m, [frames], trimaps=[tri], stabilise=True)
    finally:
        handle.remove()
    assert calls == [] and Uploads.taken == 0


def test_eval_cli_masks_frame_stabilise(tmp_path, route):
    import json
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.video import run_video_matte
    m, frames_bgr, ms, _ = route
    demo = os.path.join(str(tmp_path), "demo")
    for sub in ("frames", "mask"):
        os.makedirs(os.path.join(demo, "clip", sub))
    for t in range(T_):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
        Image.fromarray(ms[t]).save(os.path.join(demo, "clip", "mask", "%04d.png" % t))
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "2", "--masks", "frame"]
    out, sj = os.path.join(str(tmp_path), "out"), os.path.join(str(tmp_path), "s.json")
    res = eval_cli.main(common + ["--out", out, "--stabilise", "--fgr", "--composite", "10,200,30", "--summary-json", sj])
    assert res["frames"] == T_
    assert json.load(open(sj))["stabilise"] == {"strength": 0.5, "tau_colour": 24.0, "tau_alpha": 0.5, "region": "unknown"}
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames_bgr]
    ref = run_video_matte(m, rgb, masks=ms, skip=2, max_num=5, frames_are_rgb=True, stabilise=True, new_background=(10, 200, 30))
    assert not torch.equal(ref["alpha_u8"], run_video_matte(m, rgb, masks=ms, skip=2, max_num=5, frames_are_rgb=True)["alpha_u8"])
    for t in range(T_):
        png = lambda *p: np.asarray(Image.open(os.path.join(out, *p, "clip", "%04d.png" % t)))
        assert np.array_equal(png("alpha", "test", "s4_OTVM", "pred"), ref["alpha_u8"][t].numpy()), t
        assert np.array_equal(png("fgr"), ref["fgr_u8"][t].numpy()), t
        assert np.array_equal(png("comp"), ref["comp_u8"][t].numpy()), t
    out2, sj2 = os.path.join(str(tmp_path), "out2"), os.path.join(str(tmp_path), "s2.json")
    eval_cli.main(common + ["--out", out2, "--stabilise", "0.8", "--stabilise-taus", "12,0.25", "--stabilise-region", "all",
                            "--summary-json", sj2])
    assert json.load(open(sj2))["stabilise"] == {"strength": 0.8, "tau_colour": 12.0, "tau_alpha": 0.25, "region": "all"}
    ref2 = run_video_matte(m, rgb, masks=ms, skip=2, max_num=5, frames_are_rgb=True,
                           stabilise=dict(strength=0.8, tau_colour=12.0, tau_alpha=0.25, region="all"))
    for t in range(T_):
        a = np.asarray(Image.open(os.path.join(out2, "alpha", "test", "s4_OTVM", "pred", "clip", "%04d.png" % t)))
        assert np.array_equal(a, ref2["alpha_u8"][t].numpy()), t
    for extra, why in ((["--stabilise", "1.5"], "strength"), (["--stabilise", "--stabilise-taus", "0,1"], "positive"),
                       (["--stabilise", "--stabilise-taus", "5"], "C,A"), (["--stabilise-taus", "5,1"], "belong to --stabilise"),
                       (["--stabilise", "--batch", "2"], "--batch"), (["--stabilise", "--viz"], "--viz")):
        with pytest.raises(SystemExit, match=why):
            eval_cli.main(common + ["--out", out] + extra)
    with pytest.raises(SystemExit, match="--demo"):
        eval_cli.main(["--data", demo, "--synthetic-weights", "--out", out, "--stabilise"])
