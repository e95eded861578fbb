"""GPU (-m gpu): the per-frame glue kernels of csrc/glue.hip through the C ABI -- otvm_preprocess, otvm_upsample4_logits3 /
otvm_upsample4_softmax3 and otvm_trimap_to_sm against their numpy restatement (tests/glue_ref.py) bit for bit, with NaN canaries in
every output buffer; otvm_fba_head_train / otvm_fba_head against the oracle's fba_fusion in float64.  Every entry also runs at a
size above grid_for's 8192 x 256 threads, where each thread takes a second turn of its grid-stride loop."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_ref as R
from tests import glue_train_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    from otvm_amd import lib
    lib.load()
    return gpu_util


def dev(G, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.DEV)


def canary(G, n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=G.DEV)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ otvm_preprocess
OFF = dict(x11=4, sq=8, sm=4, d80=12, scaled_imgs=0)                # floats: non-zero offsets that keep 16-byte alignment
DESTS = ("x11", "sq", "sm", "d80", "scaled_imgs")


def _pp_layout(case):
    H, W, Hp, Wp, lh, lw = case
    big = Hp * Wp > K.GLUE_CAP
    ld = dict(x11=4, sq=4, sm=4, d80=0) if big else dict(x11=12, sq=8, sm=8, d80=80)
    return ld, [d for d in DESTS if not (big and d == "d80")]


def _pp_expected(G, case, r, ld, dests):
    """The whole of every buffer as it must read afterwards: canaries but for the lanes the kernel owns."""
    H, W, Hp, Wp, lh, lw = case
    P = Hp * Wp
    lanes = R.preprocess_lanes(r)
    exp = {}
    for d in dests:
        if d == "scaled_imgs":
            exp[d] = dev(G, r["scaled_imgs"].reshape(-1))
            continue
        buf = np.full(OFF[d] + P * ld[d] + 16, np.nan, np.float32)
        v = buf[OFF[d]:OFF[d] + P * ld[d]].reshape(P, ld[d])
        if d == "d80":
            v[:, 64:70] = lanes[d]
        else:
            v[:, 0:4] = lanes[d]
        exp[d] = dev(G, buf)
    return exp


def _pp_run(G, case, ld, dests, src, a_d):
    from otvm_amd import lib as L
    H, W, Hp, Wp, lh, lw = case
    P = Hp * Wp
    q = L.PreprocessParams()
    q.a, q.H, q.W, q.Hp, q.Wp, q.lh, q.lw = a_d.data_ptr(), H, W, Hp, Wp, lh, lw
    for k, v in R.NORMS.items():
        setattr(q, k, (C.c_float * 3)(*v))
    keep = []
    if "fg" in src:
        keep += [dev(G, src["fg"]), dev(G, src["bg"])]
        q.fg, q.bg = keep[0].data_ptr(), keep[1].data_ptr()
    else:
        keep += [dev(G, src["fg_u8"]), dev(G, src["bg_u8"])]
        q.fg_u8, q.bg_u8, q.u8_rgb = keep[0].data_ptr(), keep[1].data_ptr(), int(src["u8_rgb"])
    out = {}
    for d in dests:
        if d == "scaled_imgs":
            out[d] = canary(G, 3 * H * W)
            q.scaled_imgs = out[d].data_ptr()
        else:
            out[d] = canary(G, OFF[d] + P * ld[d] + 16)
            setattr(q, d, out[d].data_ptr() + 4 * OFF[d])
            setattr(q, d + "_ld", ld[d])
    L.check(L.load().otvm_preprocess(C.byref(q), G.stream()), "preprocess")
    torch.cuda.synchronize()
    return out


def _routes(fg, bg):
    return (("f32 planes", dict(fg=K.planes_f32(fg), bg=K.planes_f32(bg))),
            ("u8 bgr", dict(fg_u8=fg, bg_u8=bg, u8_rgb=False)),
            ("u8 rgb", dict(fg_u8=fg[..., ::-1].copy(), bg_u8=bg[..., ::-1].copy(), u8_rgb=True)))


@pytest.mark.parametrize("case", K.PREPROCESS, ids=K.ids(K.PREPROCESS))
def test_preprocess_routes_lanes_and_padding_equal_the_restatement(G, case):
    """fp32 BGR planes, uint8 BGR and uint8 RGB (fed the channel-reversed bytes) give the same bits, and those are the restatement's;
    the written lanes are exactly x11[0..3] (lane 3 = 0), sq / sm[0..3] and d80[64..69]: every other float keeps its canary."""
    H, W, Hp, Wp, lh, lw = case
    a, fg, bg = K.preprocess_inputs(H, W, seed=H + W)
    ld, dests = _pp_layout(case)
    r = R.preprocess(a, Hp, Wp, lh, lw, fg_u8=fg, bg_u8=bg, u8_rgb=False)
    exp = _pp_expected(G, case, r, ld, dests)
    a_d = dev(G, a)
    for name, src in _routes(fg, bg):
        out = _pp_run(G, case, ld, dests, src, a_d)
        for d in dests:
            assert same_bits(out[d], exp[d]), (name, d)


@pytest.mark.parametrize("case", K.PREPROCESS[:3], ids=K.ids(K.PREPROCESS[:3]))
def test_preprocess_each_destination_is_optional(G, case):
    """A destination given as NULL leaves the others' bits as they were."""
    H, W, Hp, Wp, lh, lw = case
    a, fg, bg = K.preprocess_inputs(H, W, seed=H + W)
    ld, dests = _pp_layout(case)
    exp = _pp_expected(G, case, R.preprocess(a, Hp, Wp, lh, lw, fg_u8=fg, bg_u8=bg), ld, dests)
    a_d = dev(G, a)
    for name, src in _routes(fg, bg)[:2]:
        for drop in dests:
            rest = [d for d in dests if d != drop]
            out = _pp_run(G, case, ld, rest, src, a_d)
            for d in rest:
                assert same_bits(out[d], exp[d]), (name, "without " + drop, d)
        for only in dests:
            out = _pp_run(G, case, ld, [only], src, a_d)
            assert same_bits(out[only], exp[only]), (name, "only " + only)


def test_preprocess_refuses_bad_arguments(G):
    """No destination at all, a view that is not 16-byte aligned, a stride that is no multiple of 4: non-zero, nothing written."""
    from otvm_amd import lib as L
    lib = L.load()
    H, W = 8, 8
    a, fg, bg = K.preprocess_inputs(H, W, seed=1)
    keep = [dev(G, a), dev(G, K.planes_f32(fg)), dev(G, K.planes_f32(bg))]
    buf = canary(G, 64 * 80 + 16)

    def params():
        q = L.PreprocessParams()
        q.a, q.fg, q.bg = (t.data_ptr() for t in keep)
        q.H, q.W, q.Hp, q.Wp = H, W, H, W
        for k, v in R.NORMS.items():
            setattr(q, k, (C.c_float * 3)(*v))
        return q
    q = params()
    assert lib.otvm_preprocess(C.byref(q), G.stream()) != 0
    for dst in ("x11", "sq", "sm", "d80"):
        q = params()
        setattr(q, dst, buf.data_ptr() + 4)
        setattr(q, dst + "_ld", 12)
        assert lib.otvm_preprocess(C.byref(q), G.stream()) != 0, dst + " misaligned"
        q = params()
        setattr(q, dst, buf.data_ptr())
        setattr(q, dst + "_ld", 6)
        assert lib.otvm_preprocess(C.byref(q), G.stream()) != 0, dst + " stride"
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# A grid-stride loop is right with any grid: were grid_for to launch one block, every value above would stay as it is and only the
# time would change.  So the cap's other half -- that a frame above it still gets 8192 blocks -- is pinned as a rate.  One block is one
# of 256 compute units, which streams at most about 90 GB/s; the whole chip reaches about 6,300 GB/s.  The floor is 200 GB/s.
GRID_FLOOR_GBPS = 200.0


def test_preprocess_above_the_cap_still_fills_the_chip(G):
    from otvm_amd import lib as L
    lib = L.load()
    case = K.PREPROCESS[-1]
    H, W, Hp, Wp, lh, lw = case
    a, fg, bg = K.preprocess_inputs(H, W, seed=H + W)
    keep = [dev(G, a), dev(G, fg), dev(G, bg)]
    P = Hp * Wp
    out = [canary(G, P * 4) for _ in range(3)] + [canary(G, 3 * H * W)]
    q = L.PreprocessParams()
    q.a, q.fg_u8, q.bg_u8, q.u8_rgb = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0
    q.H, q.W, q.Hp, q.Wp, q.lh, q.lw = case
    for k, v in R.NORMS.items():
        setattr(q, k, (C.c_float * 3)(*v))
    q.x11, q.sq, q.sm, q.scaled_imgs = (t.data_ptr() for t in out)
    q.x11_ld = q.sq_ld = q.sm_ld = 4
    nbytes = H * W * (4 + 6 + 12) + P * 48                        # alpha, two byte triples, the composite; three 16-byte stores
    rate = G.best_gbps(lambda: L.check(lib.otvm_preprocess(C.byref(q), G.stream()), "preprocess"), nbytes)
    print("glue margin preprocess %dx%d: %.0f GB/s of its %.0f MB, floor %.0f GB/s" % (Wp, Hp, rate, nbytes / 1e6, GRID_FLOOR_GBPS))
    assert rate >= GRID_FLOOR_GBPS


# ------------------------------------------------------------------------------------------------ otvm_upsample4_*
def _interleave(G, lg, ld):
    """[3, h4, w4] -> the device's [h4 * w4, ld] with NaN in the lanes that are not logits."""
    _, h4, w4 = lg.shape
    buf = np.full((h4 * w4, ld), np.nan, np.float32)
    buf[:, :3] = lg.reshape(3, -1).T
    return dev(G, buf)


def _upsample(G, lg, ld):
    from otvm_amd import lib as L
    lib = L.load()
    _, h4, w4 = lg.shape
    P = 16 * h4 * w4
    src = _interleave(G, lg, ld)
    lo, pr = canary(G, 3 * P + 4), canary(G, 3 * P + 4)
    L.check(lib.otvm_upsample4_logits3(src.data_ptr(), h4, w4, ld, lo.data_ptr(), G.stream()), "upsample4_logits3")
    L.check(lib.otvm_upsample4_softmax3(src.data_ptr(), h4, w4, ld, pr.data_ptr(), G.stream()), "upsample4_softmax3")
    torch.cuda.synchronize()
    assert bool(torch.isnan(lo[3 * P:]).all()) and bool(torch.isnan(pr[3 * P:]).all())
    return lo[:3 * P].reshape(3, 4 * h4, 4 * w4), pr[:3 * P].reshape(3, 4 * h4, 4 * w4)


@pytest.mark.parametrize("h4,w4,ld", K.UPSAMPLE, ids=K.ids(K.UPSAMPLE))
def test_upsample4_logits_equal_the_restatement_and_softmax_follows(G, h4, w4, ld):
    """The logits bit for bit; the probabilities within 2e-6 (test_fba_head's bound for the same softmax) of a float64 softmax of the
    restated logits, which leaves expf and the division as the only difference."""
    lg = K.logits(h4, w4, 8.0, seed=h4 * 100 + w4)
    lo, pr = _upsample(G, lg, ld)
    want = R.upsample4_logits(lg)
    assert same_bits(lo, dev(G, want))
    d = float((pr.double() - dev(G, R.softmax3_f64(want))).abs().max())
    print("glue margin upsample4_softmax3 %dx%d ld %d: probabilities %.3e of 2e-6" % (h4, w4, ld, d))
    assert d <= 2e-6


def test_upsample4_softmax_of_saturated_logits_is_finite(G):
    g = np.random.default_rng(3)
    lg = np.where(g.random((3, 5, 7)) < 0.5, np.float32(-80), np.float32(80)).astype(np.float32)
    lo, pr = _upsample(G, lg, 4)
    assert same_bits(lo, dev(G, R.upsample4_logits(lg)))
    assert bool(torch.isfinite(pr).all()) and float(pr.min()) >= 0.0
    assert float((pr.double().sum(0) - 1.0).abs().max()) <= 2e-6
    assert float((pr.double() - dev(G, R.softmax3_f64(R.upsample4_logits(lg)))).abs().max()) <= 2e-6


# ------------------------------------------------------------------------------------------------ otvm_trimap_to_sm
@pytest.mark.parametrize("P", K.TRIMAP_TO_SM)
def test_trimap_to_sm_writes_lanes_3_and_4_only(G, P):
    from otvm_amd import lib as L
    tri = np.random.default_rng(P).random((3, P), dtype=np.float32)
    sm = canary(G, P * 8 + 8)
    tri_d = dev(G, tri)
    L.check(L.load().otvm_trimap_to_sm(tri_d.data_ptr(), P, sm.data_ptr(), 8, G.stream()), "trimap_to_sm")
    torch.cuda.synchronize()
    want = R.trimap_to_sm(tri, np.full((P, 8), np.nan, np.float32))
    assert same_bits(sm[:P * 8].reshape(P, 8), dev(G, want)) and bool(torch.isnan(sm[P * 8:]).all())


# ------------------------------------------------------------------------------------------------ the FBA heads
def _head_case(n_out, P):
    """The 37 x 41 random pixels of test_fba_head; a larger P repeats them (period 1517, which divides neither the block nor the
    grid's stride), so that the bound below -- set for those pixels -- holds at the size above the cap as well.  Over 2,100,800
    independent random pixels float32 arithmetic itself is farther from float64 than 2e-6 in alpha (the division by den + 0.1
    amplifies up to tenfold): torch's float32 statement 3.5e-6, the kernel 4.6e-6, the six F / B planes below 1e-6."""
    from tests.test_gpu_kernels import rnd
    P0 = min(P, 37 * 41)
    hid = rnd(P0, 16, seed=50)
    w, b = rnd(n_out, 16, seed=51, scale=0.4), rnd(n_out, seed=52, scale=0.3)
    img = torch.rand(P0, 3, generator=torch.Generator().manual_seed(53))
    return hid, w, b, img, torch.arange(P) % P0


def _head_reference(hid, w, b, img):
    """float64: the 1x1 conv, clamp / sigmoid, oracle.otvm_oracle.fba_fusion -> out7 [7, P], logits [3, P] or None."""
    from oracle.otvm_oracle import fba_fusion
    o = (hid.double() @ w.double().T + b.double()).T[None, :, :, None]             # [1, n_out, P, 1]
    im = img.double().T[None, :, :, None]
    al, Fn, Bn = fba_fusion(torch.clamp(o[:, 0:1], 0, 1), im, torch.sigmoid(o[:, 1:4]), torch.sigmoid(o[:, 4:7]))
    out7 = torch.cat([al, Fn, Bn], 1)[0, :, :, 0]
    return out7, (o[0, 7:10, :, 0] if w.shape[0] == 10 else None)


@pytest.mark.parametrize("P", K.HEAD_P)
@pytest.mark.parametrize("n_out", [7, 10])
def test_fba_head_train_all_planes_and_logits(G, n_out, P):
    """All seven planes of out7 (alpha, the fused F, the fused B) within 2e-6 of fba_fusion in float64 on the float64 1x1 conv; the
    raw logits within 2^-22 max(1, max|ref|); plane 0 is otvm_fba_head's alpha bit for bit; otvm_fba_head's probabilities and its
    sm lanes 3..5 hold at the size above the grid cap as at the small one."""
    from otvm_amd import lib as L
    lib = L.load()
    hid, w, b, img, idx = _head_case(n_out, P)
    want7, want_lg = _head_reference(hid, w, b, img)
    hid, img, want7 = hid[idx], img[idx], want7[:, idx]
    want_lg = want_lg[:, idx] if n_out == 10 else None
    hid_ld, img_ld, sm_ld = (24, 8, 24) if P < K.GLUE_CAP else (16, 4, 8)
    hd = torch.full((P, hid_ld), float("nan"))
    hd[:, :16] = hid
    im = torch.full((P, img_ld), float("nan"))
    im[:, :3] = img
    hd, im, wd, bd = hd.to(G.DEV), im.to(G.DEV), w.contiguous().to(G.DEV), b.to(G.DEV)
    out7, lg = canary(G, 7 * P + 4), canary(G, 3 * P + 4)
    L.check(lib.otvm_fba_head_train(hd.data_ptr(), hid_ld, wd.data_ptr(), bd.data_ptr(), n_out, im.data_ptr(), img_ld, P,
                                    out7.data_ptr(), lg.data_ptr() if n_out == 10 else 0, G.stream()), "fba_head_train")
    alpha, tri, sm = canary(G, 2 * P), canary(G, 3 * P + 4), canary(G, P * sm_ld + 4)
    L.check(lib.otvm_fba_head(hd.data_ptr(), hid_ld, wd.data_ptr(), bd.data_ptr(), n_out, im.data_ptr(), img_ld, P, alpha.data_ptr(), 2,
                              tri.data_ptr() if n_out == 10 else 0, sm.data_ptr() if n_out == 10 else 0, sm_ld, G.stream()), "fba_head")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out7[7 * P:]).all()) and bool(torch.isnan(alpha[1::2]).all())
    got7 = out7[:7 * P].reshape(7, P)
    d7 = (got7.double() - want7.to(G.DEV)).abs().amax(1).tolist()
    print("glue margin fba_head_train n_out %d P %d: out7 planes %s of 2e-6" % (n_out, P, " ".join("%.2e" % v for v in d7)))
    assert max(d7) <= 2e-6, d7
    assert same_bits(got7[0], alpha[0::2].contiguous())
    if n_out == 7:
        assert bool(torch.isnan(lg).all())                        # no logits without the three extra outputs
        return
    assert bool(torch.isnan(lg[3 * P:]).all()) and bool(torch.isnan(tri[3 * P:]).all())
    top = max(1.0, float(want_lg.abs().max()))
    dl = float((lg[:3 * P].reshape(3, P).double() - want_lg.to(G.DEV)).abs().max())
    print("glue margin fba_head_train n_out %d P %d: logits %.3e of %.3e" % (n_out, P, dl, 2.0 ** -22 * top))
    assert dl <= 2.0 ** -22 * top
    p = torch.softmax(want_lg, 0).to(G.DEV)
    t = tri[:3 * P].reshape(3, P)
    s = sm[:P * sm_ld].reshape(P, sm_ld)
    dp = float((t.double() - p).abs().max())
    print("glue margin fba_head n_out %d P %d: probabilities %.3e of 2e-6" % (n_out, P, dp))
    assert dp <= 2e-6
    assert same_bits(s[:, 3].contiguous(), t[1]) and same_bits(s[:, 4].contiguous(), t[2]) and same_bits(s[:, 5].contiguous(), got7[0])
    others = [k for k in range(sm_ld) if k not in (3, 4, 5)]
    assert bool(torch.isnan(s[:, others]).all()) and bool(torch.isnan(sm[P * sm_ld:]).all())
