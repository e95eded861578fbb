"""GPU (-m gpu): otvm_conv2d_up -- a 3x3 patch conv whose leading input channels are the 2x bilinear upsampling of a
source-resolution tensor, interpolated while the conv stages its patch -- against the route it replaces: otvm_upsample_bilinear_b
into channels [0, Cu) of a concatenated buffer, then otvm_conv2d.  The outputs must be EQUAL (torch.equal): same source
normalisation, same blend, same split, same products in the same order.  Fused GroupNorm sums are accumulated by fp64 atomics in
an order that differs from launch to launch: they are compared as tests/test_gpu_kernels.py compares fused sums (1e-5 of the largest
sum), the table the last workgroup derives from them to two fp32 ulps of its largest entry.

The frame-level tests run whole frames with the decoder's two upsampling passes folded (OTVM_FOLD_UPSAMPLE = 2) and kept (0)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LEAKY = 2


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


def build(G, Hi, Wi, Cu, side, Cout, prec, table, epi, B, side_slice, H=None, W=None):
    """Both routes' parameter blocks over the same tensors.  Returns a dict; nothing is launched."""
    from otvm_amd import lib as L
    from otvm_amd.engine import Act, conv_params
    dev = G.DEV
    H, W = (2 * Hi, 2 * Wi) if H is None else (H, W)
    Cin = Cu + side
    src = Act(rnd(B * Hi * Wi * Cu, seed=11).to(dev), Hi, Wi, Cu, B=B, bs=Hi * Wi * Cu)
    tab = None
    if table:       # per image: [scale Cu | shift Cu]
        tab = torch.cat([1.0 + 0.3 * rnd(B, Cu, seed=12), 0.5 * rnd(B, Cu, seed=13)], 1).contiguous().to(dev)
    wide_ld, wide_off = (80, 64) if side_slice else (side, 0)
    wide = Act(rnd(B * H * W * wide_ld, seed=14).to(dev), H, W, side, wide_ld, wide_off, B=B, bs=H * W * wide_ld)
    cat = Act(torch.full((B * H * W * Cin,), float("nan"), device=dev), H, W, Cin, B=B, bs=H * W * Cin)
    for b in range(B):
        cat.ch(Cu, side).torch(b).copy_(wide.torch(b))
    w = rnd(Cout, Cin, 3, 3, seed=15, scale=1.0 / math.sqrt(Cin * 9))
    cw = G.pack_weight(w)
    assert cw.I_pad == Cin and cw.w_frag is not None
    bias = rnd(Cout, seed=16).to(dev)
    outs = [Act(torch.full((B * H * W * Cout,), float("nan"), device=dev), H, W, Cout, B=B, bs=H * W * Cout) for _ in range(2)]
    keep = [src, tab, wide, cat, cw, bias, outs]
    ps = []
    for out in outs:
        p = conv_params(cat, cw, out, bias, 1, 1, 1, LEAKY if epi == "bias_leaky" else 0, 0, None, prec)
        if epi == "gn":
            st = torch.zeros(B * 64, dtype=torch.float64, device=dev)
            gam, bet = (1.0 + 0.2 * rnd(Cout, seed=17)).to(dev), rnd(Cout, seed=18).to(dev)
            tb = torch.full((B, 2 * Cout), float("nan"), device=dev)
            cnt = torch.zeros(B, dtype=torch.int32, device=dev)
            p.gn_stats, p.gn_bs = st.data_ptr(), 64
            p.gn_gamma, p.gn_beta = gam.data_ptr(), bet.data_ptr()
            p.gn_scale_out, p.gn_shift_out, p.gn_counter, p.gn_tab_bs = tb.data_ptr(), tb.data_ptr() + 4 * Cout, cnt.data_ptr(), 2 * Cout
            keep += [st, gam, bet, tb, cnt]
            p._gn = (st, tb)
        ps.append(p)
    p_pass, p_fold = ps
    p_fold.inp, p_fold.in_ld, p_fold.in_bs = wide.ptr, wide.ld, wide.bs
    u = L.ConvUpParams()
    u.src, u.Hi, u.Wi, u.Cu, u.src_ld, u.src_bs = src.ptr, Hi, Wi, Cu, src.ld, src.bs
    if table:
        u.scale, u.shift, u.act, u.norm_bs = tab.data_ptr(), tab.data_ptr() + 4 * Cu, LEAKY, 2 * Cu
    return dict(lib=L.load(), L=L, src=src, tab=tab, cat=cat, outs=outs, p_pass=p_pass, p_fold=p_fold, u=u, keep=keep, B=B, Cu=Cu)


def run_both(G, c):
    lib, L, src, cat, u, B = c["lib"], c["L"], c["src"], c["cat"], c["u"], c["B"]
    up = cat.ch(0, c["Cu"])
    st = G.stream()
    assert lib.otvm_conv2d_accepts_upsampled_input(C.byref(c["p_fold"]), C.byref(u)) == 1
    L.check(lib.otvm_upsample_bilinear_b(src.ptr, src.H, src.W, src.C, src.ld, u.scale, u.shift, u.act, 0, 0, up.ptr, up.H, up.W, up.ld,
                                         B, src.bs, 0, up.bs, u.norm_bs, st), "upsample")
    L.check(lib.otvm_conv2d(C.byref(c["p_pass"]), st), "conv2d")
    L.check(lib.otvm_conv2d_up(C.byref(c["p_fold"]), C.byref(u), st), "conv2d_up")
    torch.cuda.synchronize()
    a, b = c["outs"][0].t, c["outs"][1].t
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), "folded conv differs from pass + conv: max |d| = %g at %d elements" % (
        float((a - b).abs().nan_to_num(float("inf")).max()), int((a != b).sum()))
    if hasattr(c["p_pass"], "_gn"):
        (s0, t0), (s1, t1) = c["p_pass"]._gn, c["p_fold"]._gn
        assert float((s0 - s1).abs().max()) <= 1e-5 * float(s0.abs().max())
        assert torch.isfinite(t0).all() and float((t0 - t1).abs().max()) <= 2 * 2.0 ** -23 * float(t0.abs().max())


F16X3, F16 = 1, 2
# Hi, Wi, Cu, side channels, side as channels 64..79 of an 80-wide buffer, Cout, source table + LeakyReLU, epilogue, batch, tile_rows
CASES = [
    # 64-filter tile; two tile rows and columns, the last ones partial; all four clamped borders; three source stages; batch 2, per-image tables
    pytest.param(5, 19, 48, 16, True, 64, True, "gn", 2, 0, id="5x19_c48+16of80_n64_tab_gn_b2"),
    # Hi = 1: both fine rows come from one source row; one source stage; no table; bias + LeakyReLU
    pytest.param(1, 16, 16, 32, False, 64, False, "bias_leaky", 1, 0, id="1x16_c16+32_n64_plain_bias"),
    # 32-filter 16x32 tile (forced: the map is far below the size at which otvm_conv2d picks it; the tiles share one summation order),
    # partial second tile both ways
    pytest.param(9, 17, 48, 16, True, 32, True, "bias_leaky", 1, 16, id="9x17_c48+16of80_n32_rows16_tab_bias"),
    # ... and the 8x32 32-filter tile otvm_conv2d runs at this size
    pytest.param(9, 17, 16, 32, False, 32, False, "bias_leaky", 2, 0, id="9x17_c16+32_n32_rows8_plain_bias_b2"),
    # exactly one tile: the halo lies entirely outside the image
    pytest.param(4, 16, 16, 32, False, 64, True, "gn", 1, 0, id="4x16_c16+32_n64_tab_gn"),
    pytest.param(4, 16, 48, 16, True, 32, True, "bias_leaky", 1, 16, id="4x16_c48+16of80_n32_rows16_tab_bias"),
]


@pytest.mark.parametrize("prec", [F16X3, F16], ids=["f16x3", "f16"])
@pytest.mark.parametrize("Hi,Wi,Cu,side,side_slice,Cout,table,epi,B,rows", CASES)
def test_conv2d_up_equals_upsample_then_conv(G, Hi, Wi, Cu, side, side_slice, Cout, table, epi, B, rows, prec):
    c = build(G, Hi, Wi, Cu, side, Cout, prec, table, epi, B, side_slice)
    c["u"].tile_rows = rows
    run_both(G, c)


def test_probe_refuses_what_the_kernel_does_not_take(G):
    """Cu = 8, a 3x map, the 256-filter wide tile, an unaligned source, a fused input normalisation: refused by the probe, and
    otvm_conv2d_up returns an error without launching (the output keeps its NaN fill)."""
    def refused(c):
        lib = c["lib"]
        assert lib.otvm_conv2d_accepts_upsampled_input(C.byref(c["p_fold"]), C.byref(c["u"])) == 0
        assert lib.otvm_conv2d_up(C.byref(c["p_fold"]), C.byref(c["u"]), G.stream()) != 0
        torch.cuda.synchronize()
        assert torch.isnan(c["outs"][1].t).all()

    c = build(G, 4, 16, 16, 16, 64, F16X3, True, "bias_leaky", 1, False)
    assert c["lib"].otvm_conv2d_accepts_upsampled_input(C.byref(c["p_fold"]), C.byref(c["u"])) == 1
    c["u"].Cu = 8
    refused(c)
    c = build(G, 4, 16, 16, 16, 64, F16X3, True, "bias_leaky", 1, False, H=12, W=48)             # 3x the source
    refused(c)
    c = build(G, 4, 16, 16, 16, 256, F16X3, True, "bias_leaky", 1, False)                        # the wide tile's layers
    refused(c)
    c = build(G, 4, 16, 16, 16, 64, F16X3, True, "bias_leaky", 1, False)
    c["u"].src = c["u"].src + 4                                                                  # not 16-byte aligned
    refused(c)
    c = build(G, 4, 16, 16, 16, 64, F16X3, True, "bias_leaky", 1, False)
    c["p_fold"].in_scale, c["p_fold"].in_shift = c["tab"].data_ptr(), c["tab"].data_ptr() + 64
    refused(c)
    c = build(G, 4, 16, 16, 16, 64, F16X3, True, "bias_leaky", 1, False)
    c["u"].tile_rows = 16                                                                        # the 16-row tile is the 32-filter layers'
    refused(c)


# ---------------------------------------------------------------- frame level
FIVE = ("alpha", "alpha_u8", "trimap", "fgr_u8", "comp_u8")


def _matte(synth_sd, fold, clips, tris, batch, tune=True):
    """Fresh model + engine with graphs on and engine.FOLD_UPSAMPLE = fold; the tuner's choices are shared through the process-wide
    cache (what a shared tune file gives two processes), so both settings launch every other layer in the same configuration."""
    from otvm_amd import engine, helpers
    from otvm_amd.video import run_video_matte, run_video_matte_batch
    old = engine.FOLD_UPSAMPLE, engine.AUTOTUNE
    engine.FOLD_UPSAMPLE, engine.AUTOTUNE = fold, tune
    try:
        cfg = helpers.default_cfg()
        m = helpers.get_model_alpha(cfg, helpers.get_model_trimap(cfg, "Test", 12), "Test", 12)
        m.load_state_dict(synth_sd, strict=True)
        m = m.cuda().eval()
        m._get_engine().use_graphs = True
        kw = dict(skip=2, max_num=3, foreground=True)
        if batch:
            res = run_video_matte_batch(m, clips, trimaps=tris, new_background=[(16, 200, 90)] * len(clips), **kw)
        else:
            res = [run_video_matte(m, clips[0], trimap=tris[0], new_background=(16, 200, 90), **kw)]
        pl = m._engine.last_plan
        assert len(pl.graphs) >= 4                                   # the lists were captured and replayed
        return res, dict(pl.upfold_routes)
    finally:
        engine.FOLD_UPSAMPLE, engine.AUTOTUNE = old


@pytest.mark.parametrize("H,W,batch", [(70, 90, False), (100, 150, False), (70, 90, True)], ids=["70x90", "100x150", "70x90_batch2"])
def test_frames_folded_equal_frames_with_the_upsampling_passes(G, synth_sd, H, W, batch):
    """Three frames, every output of every frame: OTVM_FOLD_UPSAMPLE = 2 (both decoder maps read at source resolution wherever the
    library takes their readers) against 0 (the passes), captured graphs replaying the chosen route.  The single-clip cases run
    with the plan-time tuner (a reader it moved to an implicit-GEMM tile keeps its pass); the lock-step batch runs the built-in
    heuristic, under which every reader is a patch conv and both maps (u2 and u3) must be folded."""
    from otvm_amd.synth_data import synthetic_clip
    pairs = [synthetic_clip(H, W, 3, seed=500 + b) for b in range(2 if batch else 1)]
    clips, tris = [p[0] for p in pairs], [p[1] for p in pairs]
    folded, routes2 = _matte(synth_sd, 2, clips, tris, batch, tune=not batch)
    passes, routes0 = _matte(synth_sd, 0, clips, tris, batch, tune=not batch)
    print("routes with OTVM_FOLD_UPSAMPLE=2:", routes2)
    assert routes0 and not any(routes0.values())
    assert any(routes2.values()), routes2                            # the comparison below is about something
    if batch:
        assert routes2["NET.decoder.conv_up2.1"] == 1 and routes2["NET.decoder.conv_up3.1"] == 1, routes2
    for b, (x, y) in enumerate(zip(folded, passes)):
        for k in FIVE:
            assert torch.equal(x[k], y[k]), "clip %d, %s" % (b, k)
