"""GPU (-m gpu): the foreground outputs -- the heads' F kept by the _fgr entry points, the output kernel against its numpy
restatement (tests/fgr_ref.py) bit for bit, whole frames against the oracle and the reference's fixtures, and the proof that
nothing else moves when the option is switched."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import fgr_ref
from tests.common import GOLDEN, clip_inputs, frame_flags, load_sequences_meta

pytestmark = pytest.mark.gpu
META = load_sequences_meta()
FGR_TOL = 1e-3          # the contract of this head's outputs (stated for alpha; F leaves the same fusion, better conditioned)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    from otvm_amd import lib
    lib.load()
    return gpu_util


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ 4: the fusion vector
def test_reference_vector_fba_fusion_foreground(G):
    """ff_* of ops.npz (the reference's fba_fusion) through otvm_fba_head_fgr with the identity head, as
    test_reference_vectors_fba_fusion drives otvm_fba_head: F against ff_out[0, 1:4]."""
    from otvm_amd import lib as L
    lib = L.load()
    ops = np.load(os.path.join(GOLDEN, "ops.npz"))
    a, img, Fg, Bg = (torch.from_numpy(ops[k]) for k in ("ff_a", "ff_img", "ff_F", "ff_B"))
    want = torch.from_numpy(ops["ff_out"])
    _, _, H, W = a.shape
    P = H * W
    logit = lambda p: torch.log(p.double() / (1 - p.double())).float()
    hid = torch.zeros(1, 16, H, W)
    hid[:, 0:1], hid[:, 1:4], hid[:, 4:7] = a, logit(Fg), logit(Bg)
    wd = torch.eye(16)[:7].contiguous().to(G.DEV)
    bd = torch.zeros(7, device=G.DEV)
    ha, ia = G.to_act(hid, c_pad=16), G.to_act(img, c_pad=4)
    alpha = torch.full((P,), float("nan"), device=G.DEV)
    fgr = torch.full((3 * P,), float("nan"), device=G.DEV)
    L.check(lib.otvm_fba_head_fgr(ha.ptr, ha.ld, wd.data_ptr(), bd.data_ptr(), 7, ia.ptr, ia.ld, P, alpha.data_ptr(), 1, 0, 0, 0,
                                  fgr.data_ptr(), G.stream()))
    torch.cuda.synchronize()
    da, df = G.maxdiff(alpha.cpu(), want[0, 0].flatten()), G.maxdiff(fgr.cpu().reshape(3, P), want[0, 1:4].reshape(3, P))
    print("fusion vector: alpha %.2e F %.2e" % (da, df))
    assert da <= 5e-6 and df <= 5e-6
    assert lib.otvm_fba_head_fgr(ha.ptr, ha.ld, wd.data_ptr(), bd.data_ptr(), 7, ia.ptr, ia.ld, P, alpha.data_ptr(), 1, 0, 0, 0,
                                 0, G.stream()) != 0


# ------------------------------------------------------------------------------------------------ 5: the head routes
@pytest.mark.parametrize("batch", [1, 2], ids=["b1", "b2"])
@pytest.mark.parametrize("wide16", [False, True, "generic"], ids=["tile32", "tile16", "tile16-relu-nobias"])
@pytest.mark.parametrize("n_out,H,W,write_hid", [(7, 40, 64, False), (7, 37, 45, True), (10, 24, 96, True), (10, 19, 33, True)])
def test_head_routes_keep_the_same_foreground(G, n_out, H, W, write_hid, wide16, batch):
    """otvm_conv2d_head_fgr on the shapes of test_conv_with_head_epilogue: alpha / trimap / sm / hidden state bit-identical to
    otvm_conv2d_head; F == planes 1..3 of otvm_fba_head_train on the hidden state (bit for bit on the 32-wide route, whose
    hidden state is the one the head read; within 2e-5, the bound alpha has between the routes, on the 16-wide ones); nothing
    written outside the image."""
    from otvm_amd import lib as L
    from otvm_amd.engine import conv_params
    lib, st = L.load(), G.stream()
    P, B = H * W, batch
    generic = wide16 == "generic"
    act = 1 if generic else 2
    cw = G.pack_weight(rnd(16, 32, 3, 3, seed=81, scale=1.0 / math.sqrt(32 * 9)))
    bd = None if generic else rnd(16, seed=82, scale=0.2).to(G.DEV)
    hw, hb = rnd(n_out, 16, seed=83, scale=0.4).contiguous().to(G.DEV), rnd(n_out, seed=84, scale=0.3).to(G.DEV)
    xs = [G.to_act(rnd(1, 32, H, W, seed=80 + 7 * b)) for b in range(B)]
    ims = [G.to_act(torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(85 + b)), c_pad=4, ld=8) for b in range(B)]
    # one flat buffer per tensor, image b at b * stride (what otvm_conv_params.batch expects)
    xb = torch.cat([x.t.flatten() for x in xs]).contiguous()
    ib = torch.cat([i.t.flatten() for i in ims]).contiguous()
    x_bs, i_bs = xs[0].t.numel(), ims[0].t.numel()
    SLACK = 64

    def run(fgr_on):
        hid = torch.full((B * P * 24,), float("nan"), device=G.DEV)
        a = torch.full((B * 2 * P,), float("nan"), device=G.DEV)
        t = torch.full((B * 3 * P,), float("nan"), device=G.DEV)
        sm = torch.zeros(B * P * 24, device=G.DEV)
        fg = torch.full((B * (3 * P + SLACK),), float("nan"), device=G.DEV)
        from otvm_amd.engine import Act
        xa = Act(xb, H, W, 32, ld=xs[0].ld, B=B, bs=x_bs)
        ha = Act(hid, H, W, 16, ld=24, B=B, bs=P * 24)
        p = conv_params(xa, cw, ha, bd, 1, 1, 1, act, 0, None, 1)
        p.batch, p.in_bs, p.out_bs = B, x_bs, P * 24
        if not write_hid:
            p.out, p.out_ld, p.out_bs = 0, 0, 0
        h = L.HeadParams()
        h.w, h.b, h.n_out, h.img, h.img_ld, h.P = hw.data_ptr(), hb.data_ptr(), n_out, ib.data_ptr(), ims[0].ld, P
        h.alpha_out, h.alpha_stride = a.data_ptr(), 2
        h.img_bs, h.alpha_bs, h.tri_bs, h.sm_bs = i_bs, 2 * P, 3 * P, P * 24
        if n_out == 10:
            h.tri_out, h.sm, h.sm_ld = t.data_ptr(), sm.data_ptr() + 64, 24
        if wide16:
            h.w16 = cw.w16.data_ptr()
        if fgr_on:
            L.check(lib.otvm_conv2d_head_fgr(C.byref(p), C.byref(h), fg.data_ptr(), 3 * P + SLACK, st), "conv2d_head_fgr")
        else:
            L.check(lib.otvm_conv2d_head(C.byref(p), C.byref(h), st), "conv2d_head")
        torch.cuda.synchronize()
        return hid, a, t, sm, fg
    hid0, a0, t0, sm0, _ = run(False)
    hid1, a1, t1, sm1, fg = run(True)
    eq = lambda u, v: torch.equal(torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0))
    assert eq(a1, a0) and eq(t1, t0) and eq(sm1, sm0) and eq(hid1, hid0)
    fgv = fg.reshape(B, 3 * P + SLACK)
    assert bool(torch.isnan(fgv[:, 3 * P:]).all()), "written beyond the three planes"
    assert bool(torch.isfinite(fgv[:, :3 * P]).all())
    for b in range(B):
        tol = 0.0 if not wide16 else 2e-5       # 32-wide: bit for bit; 16-wide: the bound alpha has between the routes
        if write_hid:
            hsrc, hld = hid1[b * P * 24:(b + 1) * P * 24], 24
        else:                                   # the hidden state was not written: from the plain convolution (same tiles on
            ho = G.empty_act(H, W, 16, ld=24)   # the 32-wide route; another summation order on the 16-wide one)
            G.conv2d(xs[b], cw, ho, bd, pad=1, act=act, precision=1)
            hsrc, hld = ho.t, 24
        out7 = torch.full((7 * P,), float("nan"), device=G.DEV)
        lg = torch.empty(3 * P, device=G.DEV)
        L.check(lib.otvm_fba_head_train(hsrc.data_ptr(), hld, hw.data_ptr(), hb.data_ptr(), n_out, ims[b].ptr, ims[b].ld, P,
                                        out7.data_ptr(), lg.data_ptr() if n_out == 10 else 0, st), "fba_head_train")
        torch.cuda.synchronize()
        want = out7.reshape(7, P)[1:4].cpu()
        got = fgv[b, :3 * P].reshape(3, P).cpu()
        d = G.maxdiff(got, want)
        assert d <= tol, (b, d, tol)
        # and alpha of that training head is the fused call's alpha (the F stored is the one alpha was computed from)
        assert G.maxdiff(out7[:P].cpu(), a1[b * 2 * P:(b + 1) * 2 * P:2].cpu()) <= tol
    p_bad = L.HeadParams()
    assert lib.otvm_conv2d_head_fgr(None, C.byref(p_bad), 0, 0, st) != 0


# ------------------------------------------------------------------------------------------------ 6: the output kernel
def _planes(Hp, Wp, seed, nonfinite):
    g = np.random.default_rng(seed)
    k255 = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    def plane():
        v = g.random((Hp, Wp), dtype=np.float32)
        m = g.random((Hp, Wp)) < 0.3
        v[m] = k255[g.integers(0, 256, int(m.sum()))]               # exact k/255 values, 0 and 1 among them
        m = g.random((Hp, Wp)) < 0.05
        v[m] = np.nextafter(k255[g.integers(1, 256, int(m.sum()))], np.float32(0))
        return v
    a, F = plane(), np.stack([plane() for _ in range(3)])
    if nonfinite:
        for arr in (a, F[0], F[2]):
            idx = g.integers(0, Hp * Wp, 12)
            arr.reshape(-1)[idx] = np.array([np.nan, np.inf, -np.inf] * 4, np.float32)
    return a, F


FGR_CASES = [(37, 64, 3, 5, 64, 96), (41, 61, 4, 9, 64, 96), (30, 62, 1, 1, 32, 64), (29, 63, 2, 1, 32, 64),
             (1080, 1920, 4, 0, 1088, 1920), (2160, 3840, 8, 0, 2176, 3840)]


@pytest.mark.parametrize("H,W,lh,lw,Hp,Wp", FGR_CASES, ids=["%dx%d" % (c[1], c[0]) for c in FGR_CASES])
@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
def test_fgr_outputs_equal_the_restatement(G, H, W, lh, lw, Hp, Wp, rgb):
    from otvm_amd import lib as L
    lib, st = L.load(), G.stream()
    big = H >= 1080
    a, F = _planes(Hp, Wp, seed=H * 7 + W, nonfinite=not big or rgb)
    ad, Fd = torch.from_numpy(a).to(G.DEV), torch.from_numpy(F).to(G.DEV)
    ac, Fc = a[lh:lh + H, lw:lw + W], F[:, lh:lh + H, lw:lw + W]
    bg_img = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    bg_img[:4, :8] = 0
    bg_img[4:8, :8] = 255
    for bg in ((bg_img, (7, 130, 255)) if not (big and not rgb) else (bg_img,)):
        for request in (("fgr", "rgba", "comp"), ("rgba",), ("comp",), ("fgr",)):
            outs = dict(fgr=torch.full((3, H, W), -5.0, device=G.DEV), rgba=torch.full((H, W, 4), 77, dtype=torch.uint8, device=G.DEV),
                        comp=torch.full((H, W, 3), 77, dtype=torch.uint8, device=G.DEV))
            q = L.FgrParams()
            q.alpha_p, q.fgr_p = ad.data_ptr(), Fd.data_ptr()
            q.Hp, q.Wp, q.H, q.W, q.lh, q.lw, q.u8_rgb = Hp, Wp, H, W, lh, lw, int(rgb)
            if "fgr" in request:
                q.fgr = outs["fgr"].data_ptr()
            if "rgba" in request:
                q.rgba_u8 = outs["rgba"].data_ptr()
            if "comp" in request:
                q.comp_u8 = outs["comp"].data_ptr()
            bgd = None
            if isinstance(bg, tuple):
                q.bg_color[:] = list(bg)
            else:
                bgd = torch.from_numpy(bg).to(G.DEV)
                q.bg_u8 = bgd.data_ptr()
            L.check(lib.otvm_fgr_outputs(C.byref(q), st), "fgr_outputs")
            torch.cuda.synchronize()
            first = {k: v.clone() for k, v in outs.items()}
            L.check(lib.otvm_fgr_outputs(C.byref(q), st), "fgr_outputs")
            torch.cuda.synchronize()
            w_fgr, w_rgba, w_comp = fgr_ref.fgr_outputs(ac, Fc, bg=bg, u8_rgb=rgb)
            got = {k: v.cpu().numpy() for k, v in outs.items()}
            for k in outs:
                assert torch.equal(first[k].view(torch.uint8), outs[k].view(torch.uint8)), "two calls differ: " + k
            if "fgr" in request:
                assert np.array_equal(got["fgr"].view(np.uint32), w_fgr.view(np.uint32))
            else:
                assert (got["fgr"] == -5.0).all()
            if "rgba" in request:
                assert np.array_equal(got["rgba"], w_rgba)
            else:
                assert (got["rgba"] == 77).all()
            if "comp" in request:
                assert np.array_equal(got["comp"], w_comp)
            else:
                assert (got["comp"] == 77).all()
            if big:
                break                               # the full-size cases: every output once per background
    # the A channel is the byte otvm_crop_outputs writes (finite alpha)
    a_fin = np.nan_to_num(a, nan=0.5, posinf=0.5, neginf=0.5)
    af = torch.from_numpy(a_fin).to(G.DEV)
    al, au8 = torch.empty(H * W, device=G.DEV), torch.empty(H * W, dtype=torch.uint8, device=G.DEV)
    L.check(lib.otvm_crop_outputs(af.data_ptr(), 0, Hp, Wp, H, W, lh, lw, al.data_ptr(), au8.data_ptr(), 0, st))
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device=G.DEV)
    q = L.FgrParams()
    q.alpha_p, q.fgr_p, q.rgba_u8 = af.data_ptr(), Fd.data_ptr(), rgba.data_ptr()
    q.Hp, q.Wp, q.H, q.W, q.lh, q.lw, q.u8_rgb = Hp, Wp, H, W, lh, lw, int(rgb)
    L.check(lib.otvm_fgr_outputs(C.byref(q), st), "fgr_outputs")
    torch.cuda.synchronize()
    assert torch.equal(rgba[..., 3].cpu(), au8.reshape(H, W).cpu())
    # refused: nothing requested, no alpha for the bytes, an output that does not fit the padded frame
    q2 = L.FgrParams()
    q2.fgr_p, q2.Hp, q2.Wp, q2.H, q2.W = Fd.data_ptr(), Hp, Wp, H, W
    assert lib.otvm_fgr_outputs(C.byref(q2), st) != 0
    q2.rgba_u8 = rgba.data_ptr()
    assert lib.otvm_fgr_outputs(C.byref(q2), st) != 0
    q.lw = Wp - W + 1
    assert lib.otvm_fgr_outputs(C.byref(q), st) != 0


# ------------------------------------------------------------------------------------------------ 7: frames
def _model(sd, dk, precision="f16x3", foreground=True):
    from tests.test_gpu_frame import _fresh_model
    m = _fresh_model(sd, dk, precision)
    m.module.foreground = foreground
    return m


def _crop(pl, x):
    return x[..., pl.lh:pl.lh + pl.H, pl.lw:pl.lw + pl.W]


FRAME_CASES = [(n, "f16x3") for n in sorted(META.keys())] + [(n, "f32") for n in ("demo_100x150_s5m5", "v108_64x96_s3m3",
                                                                                    "demo_70x90_single")]


@pytest.mark.parametrize("name,precision", FRAME_CASES, ids=["%s-%s" % c for c in FRAME_CASES])
def test_foreground_vs_oracle_on_the_golden_clips(name, precision, synth_sd):
    """last_fgr of every frame against the oracle's ref7[:, 1:4] (cropped), with run_sequence's tie-break protocol."""
    from tests import test_gpu_frame as TF
    meta = META[name]
    cache = {}

    def make(dk, prec="f16x3"):
        if (dk, prec) not in cache:
            cache[(dk, prec)] = _model(synth_sd, dk, prec)
        return cache[(dk, prec)]
    got = []
    orig = TF.stage_report

    def report(pl, cap, first_frame):               # called once per frame, after the (possibly tie-broken) oracle frame
        eng = pl.e
        assert pl.fgr and eng.last_fgr is not None
        want = _crop(pl, cap["ref7"][0, 1:4])
        got.append((float((eng.last_fgr.cpu() - want).abs().max()), eng.last_fgr.cpu().numpy(), eng.last_rgba_u8.cpu().numpy()))
        return orig(pl, cap, first_frame)
    TF.stage_report = report
    try:
        res = TF.run_sequence(make, synth_sd, meta, precision=precision)
    finally:
        TF.stage_report = orig
    assert len(got) == len(res) > 0, "the foreground was not collected for every frame"
    worst = (0.0, -1, 0.0)
    for r, (d, fgr, rgba) in zip(res, got):
        if d > worst[0]:
            worst = (d, r["t"], r["alpha"])
        _, w_rgba, _ = fgr_ref.fgr_outputs(r["out"][3][0, 0, 0].cpu().numpy(), fgr)
        assert np.array_equal(rgba, w_rgba)
    print("fgr margin %s %s: worst F max-abs vs oracle %.3e at frame %d (alpha there %.3e; bound %.0e)"
          % (name, precision, worst[0], worst[1], worst[2], FGR_TOL))
    for r, (d, _, _) in zip(res, got):
        assert r["alpha"] <= TF.ALPHA_TOL
        assert d <= FGR_TOL, "frame %d: F max-abs %.3e (alpha %.3e)" % (r["t"], d, r["alpha"])


def test_foreground_vs_reference_stages(synth_sd):
    """stages_64x64.npz: the whole reference network's ref7_t[:, 1:4], two frames, directly."""
    from otvm_amd.synth_data import synthetic_clip
    g = np.load(os.path.join(GOLDEN, "stages_64x64.npz"))
    H, W = int(g["H"]), int(g["W"])
    frames, tri = synthetic_clip(H, W, 2, int(g["clip_seed"]))
    for precision in ("f16x3", "f32"):
        m = _model(synth_sd, int(g["dk"]), precision)
        for t in range(2):
            fg = torch.from_numpy(frames[t].astype(np.float32)).permute(2, 0, 1)[None, None].contiguous()
            out = m(torch.ones(1, 1, 1, H, W), fg, fg.clone(), tri_gt=torch.from_numpy(tri)[None, None], first_frame=(t == 0),
                    last_frame=False, memorize=(t == 0), max_memory_num=5, _frame_id=t)
            torch.cuda.synchronize()
            eng = m.module._engine
            pl = eng.last_plan
            ref7 = torch.from_numpy(g["ref7_%d" % t])
            d = float((eng.last_fgr.cpu() - _crop(pl, ref7[0, 1:4])).abs().max())
            da = float((out[3][0, 0].cpu() - _crop(pl, ref7[0, :1])).abs().max())
            print("fgr margin stages_64x64 %s t=%d: F max-abs vs the reference %.3e (alpha %.3e; bound %.0e)" % (precision, t, d, da, FGR_TOL))
            assert d <= FGR_TOL, (precision, t, d, da)


# ------------------------------------------------------------------------------------------------ 8: nothing else moved
def _clip(H=64, W=96, T=4, seed=23):
    from otvm_amd.synth_data import synthetic_clip
    return synthetic_clip(H, W, T, seed)


def test_option_off_on_off_changes_nothing_else(synth_sd, tmp_path, monkeypatch):
    from otvm_amd import engine
    from otvm_amd.video import run_video_matte
    monkeypatch.setenv("OTVM_TUNE_FILE", os.path.join(str(tmp_path), "tune.json"))
    frames, tri = _clip()
    m = _model(synth_sd, 12, foreground=False)
    runs = []
    for on in (False, True, False):
        kw = dict(foreground=True, new_background=(0, 255, 0)) if on else {}
        runs.append(run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, **kw))
        assert m.module.foreground is False                          # restored
    for r in (runs[0], runs[2]):
        assert sorted(r) == ["alpha", "alpha_u8", "bank_frames", "trimap"]
    assert sorted(runs[1]) == ["alpha", "alpha_u8", "bank_frames", "comp_u8", "fgr_u8", "trimap"]
    for r in runs[1:]:
        for k in ("alpha", "alpha_u8", "trimap"):
            assert torch.equal(r[k], runs[0][k]), k
        assert r["bank_frames"] == runs[0]["bank_frames"]
    assert torch.equal(runs[1]["fgr_u8"][..., 3], runs[1]["alpha_u8"])
    assert m.module._engine.last_fgr is None                         # the last run had the option off
    # the unfused route (conv + otvm_fba_head_fgr) gives the same bytes as the fused one within the routes' alpha bound
    monkeypatch.setattr(engine, "FUSE_HEAD", 0)
    m2 = _model(synth_sd, 12, foreground=False)
    r_off = run_video_matte(m2, frames, trimap=tri, skip=2, max_num=3)
    r_on = run_video_matte(m2, frames, trimap=tri, skip=2, max_num=3, foreground=True)
    for k in ("alpha", "alpha_u8", "trimap"):
        assert torch.equal(r_on[k], r_off[k]), k
    assert int((r_on["fgr_u8"].int() - runs[1]["fgr_u8"].int()).abs().max()) <= 1
    # changing the option in the middle of a clip is refused
    core = m.module
    H, W = frames[0].shape[:2]
    fg = torch.from_numpy(frames[0].astype(np.float32)).permute(2, 0, 1)[None, None].contiguous()
    args = (torch.ones(1, 1, 1, H, W), fg, fg.clone())
    core(*args, tri_gt=torch.from_numpy(tri)[None, None], first_frame=True, memorize=True, max_memory_num=3)
    core.foreground = True
    with pytest.raises(RuntimeError, match="first frame"):
        core(*args, tri_gt=torch.from_numpy(tri)[None, None], first_frame=False, memorize=False, max_memory_num=3)
    core.foreground = False


def test_foreground_graph_replay_equals_direct_launches(synth_sd):
    from otvm_amd.video import run_video_matte
    frames, tri = _clip(T=5)
    bg = np.random.default_rng(3).integers(0, 256, frames[0].shape, dtype=np.uint8)
    res = []
    for graphs in (False, True):
        m = _model(synth_sd, 12, foreground=False)
        m.module._get_engine().use_graphs = graphs
        res.append(run_video_matte(m, frames, trimap=tri, skip=2, max_num=3, foreground=True, new_background=bg))
        if graphs:
            assert m.module._engine.last_plan.graphs, "nothing was captured"
    for k in ("alpha", "alpha_u8", "trimap", "fgr_u8", "comp_u8"):
        assert torch.equal(res[0][k], res[1][k]), k


def test_foreground_batched_equals_single(synth_sd, tmp_path, monkeypatch):
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    monkeypatch.setenv("OTVM_AUTOTUNE", "0")
    from otvm_amd import engine
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    clips = [_clip(seed=23), _clip(seed=29)]
    bgs = [np.random.default_rng(3).integers(0, 256, clips[0][0][0].shape, dtype=np.uint8), (10, 200, 30)]
    m = _model(synth_sd, 12, foreground=False)
    single = [run_video_matte(m, c[0], trimap=c[1], skip=2, max_num=3, foreground=True, new_background=bgs[b])
              for b, c in enumerate(clips)]
    batched = run_video_matte_batch(m, [c[0] for c in clips], trimaps=[c[1] for c in clips], skip=2, max_num=3, foreground=True,
                                    new_background=bgs)
    off = run_video_matte_batch(m, [c[0] for c in clips], trimaps=[c[1] for c in clips], skip=2, max_num=3)
    for b in range(2):
        assert sorted(off[b]) == ["alpha", "alpha_u8", "bank_frames", "trimap"]
        for k in ("alpha", "alpha_u8", "trimap", "fgr_u8", "comp_u8"):
            assert torch.equal(batched[b][k], single[b][k]), (b, k)
        for k in ("alpha", "alpha_u8", "trimap"):
            assert torch.equal(off[b][k], single[b][k]), (b, k)
    # keep_on_device changes where the results live and nothing else: one clip over a colour, and the two-clip batch
    kept = run_video_matte(m, clips[1][0], trimap=clips[1][1], skip=2, max_num=3, foreground=True, new_background=bgs[1],
                           keep_on_device=True)
    kept_b = run_video_matte_batch(m, [c[0] for c in clips], trimaps=[c[1] for c in clips], skip=2, max_num=3, foreground=True,
                                   new_background=bgs, keep_on_device=True)
    for on_device, on_host in [(kept, single[1])] + list(zip(kept_b, batched)):
        for k in ("alpha", "alpha_u8", "trimap", "fgr_u8", "comp_u8"):
            assert on_device[k].is_cuda and not on_host[k].is_cuda, k
            assert torch.equal(on_device[k].cpu(), on_host[k]), k


def test_recomputed_first_frame_publishes_the_returned_frame(synth_sd, monkeypatch):
    """The ill-conditioned checkpoint of test_predicted_groupnorm_falls_back_when_ill_conditioned: the conditioning guard
    computes the clip's first frame twice; the foreground outputs belong to the frame that is returned."""
    from oracle.otvm_oracle import OtvmOracle
    from otvm_amd import engine
    from otvm_amd.synth_data import synthetic_clip
    from tests.test_gpu_frame import _ill_conditioned_sd
    monkeypatch.setattr(engine, "GN_PREDICT_MIN_PIXELS", 0)
    sd, blk = _ill_conditioned_sd(synth_sd)
    H, W = 64, 96
    frames, tri = synthetic_clip(H, W, 1, seed=31)
    m = _model(sd, 12)
    m.module.set_background((0, 255, 0))
    orc = OtvmOracle(sd, dilate_kernel=12)
    fg = torch.from_numpy(frames[0].astype(np.float32)).permute(2, 0, 1)[None, None].contiguous()
    a, tg = torch.ones(1, 1, 1, H, W), torch.from_numpy(tri)[None, None]
    kw = dict(first_frame=True, last_frame=False, memorize=True, max_memory_num=3)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m(a, fg, fg.clone(), tri_gt=tg, _frame_id=0, **kw)
    torch.cuda.synchronize()
    eng = m.module._engine
    assert [e for e in eng.gn_predict_log if e[0] == blk], "the guard did not intervene: the first frame was not recomputed"
    cap = {}
    orc.frame(a, fg, fg.clone(), tri_gt=tg, frame_id=0, capture=cap, **kw)
    pl = eng.last_plan
    d = float((eng.last_fgr.cpu() - _crop(pl, cap["ref7"][0, 1:4])).abs().max())
    print("fgr margin ill-conditioned checkpoint frame 0: F max-abs vs oracle %.3e (bound %.0e)" % (d, FGR_TOL))
    assert d <= FGR_TOL, d
    _, w_rgba, w_comp = fgr_ref.fgr_outputs(out[3][0, 0, 0].cpu().numpy(), eng.last_fgr.cpu().numpy(), bg=(0, 255, 0))
    assert np.array_equal(eng.last_rgba_u8.cpu().numpy(), w_rgba) and np.array_equal(eng.last_comp_u8.cpu().numpy(), w_comp)
    assert torch.equal(eng.last_rgba_u8[..., 3], eng.last_alpha_u8)


def test_poisoned_foreground_raises_under_check_finite(synth_sd):
    m = _model(synth_sd, 12)
    frames, tri = _clip(T=1)
    H, W = frames[0].shape[:2]
    fg = torch.from_numpy(frames[0].astype(np.float32)).permute(2, 0, 1)[None, None].contiguous()
    eng = m.module._get_engine()
    eng.check_finite = True
    real = eng._fgr_outputs

    def poisoned(pl, outs, H_, W_, rgb, stream):
        real(pl, outs, H_, W_, rgb, stream)
        eng.last_fgr_b[0][1, 3, 4] = float("nan")
    eng._fgr_outputs = poisoned
    with pytest.raises(FloatingPointError, match="foreground"):
        m(torch.ones(1, 1, 1, H, W), fg, fg.clone(), tri_gt=torch.from_numpy(tri)[None, None], first_frame=True, last_frame=True,
          memorize=False, max_memory_num=3)


# ------------------------------------------------------------------------------------------------ 9: drivers
def test_eval_cli_writes_foreground_and_composite(tmp_path, synth_sd):
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.video import run_video_matte
    H, W, T = 64, 96, 3
    frames_bgr, tri = _clip(H, W, T, seed=41)
    demo = os.path.join(str(tmp_path), "demo")
    os.makedirs(os.path.join(demo, "clip", "frames")); os.makedirs(os.path.join(demo, "clip", "trimap"))
    for t in range(T):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
    Image.fromarray((np.asarray(tri)[1] * 128 + np.asarray(tri)[2] * 255).astype(np.uint8)).save(
        os.path.join(demo, "clip", "trimap", "0000.png"))
    out0, out1, out2 = (os.path.join(str(tmp_path), n) for n in ("plain", "fgr", "fgr_sync"))
    bg_path = os.path.join(str(tmp_path), "new_bg.png")
    bg_small = np.random.default_rng(9).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    bg_small[..., 0] //= 4                                   # a red-poor image: a channel swap would show
    Image.fromarray(bg_small).save(bg_path)
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "2"]
    assert eval_cli.main(common + ["--out", out0])["frames"] == T
    # prefetcher route (RGB frames on the device) over an asymmetric colour given as R,G,B
    assert eval_cli.main(common + ["--out", out1, "--fgr", "--composite", "10,200,30"])["frames"] == T
    # --sync-io route (decoded B, G, R frames: colour / image / PNG channels are flipped on the host) over an image
    assert eval_cli.main(common + ["--out", out2, "--sync-io", "--fgr", "--composite", bg_path])["frames"] == T
    assert not os.path.exists(os.path.join(out0, "fgr")) and not os.path.exists(os.path.join(out0, "comp"))
    m = _model(synth_sd, 12, foreground=False)
    rgb = [np.ascontiguousarray(f[..., ::-1]) for f in frames_bgr]
    from otvm_amd.datasets import Demo_Test, load_sequence
    d = load_sequence(next(iter(Demo_Test(demo))))
    ref = run_video_matte(m, rgb, trimap=d["trimap"], skip=2, max_num=5, frames_are_rgb=True, foreground=True,
                          new_background=(10, 200, 30))
    bg_full = np.asarray(Image.open(bg_path).convert("RGB").resize((W, H), Image.BILINEAR))
    ref_img = run_video_matte(m, rgb, trimap=d["trimap"], skip=2, max_num=5, frames_are_rgb=True, new_background=bg_full)
    assert not np.array_equal(ref["comp_u8"].numpy()[..., 0], ref["comp_u8"].numpy()[..., 2])
    for t in range(T):
        n = "%04d.png" % t
        pa = [open(os.path.join(o, "alpha", "test", "s4_OTVM", "pred", "clip", n), "rb").read() for o in (out0, out1)]
        assert pa[0] == pa[1]
        assert np.array_equal(np.asarray(Image.open(os.path.join(out2, "alpha", "test", "s4_OTVM", "pred", "clip", n))),
                              ref["alpha_u8"][t].numpy())
        f = Image.open(os.path.join(out1, "fgr", "clip", n))
        c = Image.open(os.path.join(out1, "comp", "clip", n))
        assert f.mode == "RGBA" and c.mode == "RGB"
        assert np.array_equal(np.asarray(f), ref["fgr_u8"][t].numpy())
        assert np.array_equal(np.asarray(c), ref["comp_u8"][t].numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(out2, "fgr", "clip", n))), ref_img["fgr_u8"][t].numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(out2, "comp", "clip", n))), ref_img["comp_u8"][t].numpy())
    with pytest.raises(SystemExit):
        eval_cli.main(common + ["--out", out1, "--fgr", "--batch", "2"])
