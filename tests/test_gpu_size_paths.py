"""GPU (-m gpu): the kernels whose code path or accumulation depth is picked from the image size, checked on EVERY element at
the sizes that select each path (the small-shape tests of test_gpu_kernels.py all run the path of the smallest sizes):
  - trimap encoding: the exact EDT's column pass (edt_columns_kernel<8|20|40>, edt_columns_tall_kernel) and the row pass's
    far field, with the integer squared distance recovered from the encoded channel and required to be exact;
  - f16x3 memory read: chunks of several 64-row tiles that cross slot boundaries, the engine's two-step partial/combine
    sequence and an all-singletons grouping, against softmax(K q / sqrt(128)) V in float64 over all queries;
  - GroupNorm statistics (otvm_gn_stats and the fused conv epilogue) at full resolution with a large per-group mean.
The case lists and the restated selection rules live in tests/size_paths.py; tests/test_host_logic.py checks (without a GPU)
that the cases reach every path, so a retuned threshold cannot silently move them back onto the covered one."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.size_paths import EDT_CASES, MR_SHAPES, mr_launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    from otvm_amd import lib
    lib.load()
    return gpu_util


# --------------------------------------------------------------------------------------------------- trimap encoding
DEN2 = 2.0 * (0.16 * 320) ** 2       # exp(-d^2 / DEN2): the sigma = 0.16 channel of either class


def _onehot(lab):
    return F.one_hot(lab.long(), 3).permute(2, 0, 1).float().contiguous()


def _edt_probs(Hp, Wp, pat, seed=0):
    """[3, Hp, Wp] class probabilities; labels 0 = bg, 1 = unknown, 2 = fg (the EDT runs for bg and for fg pixels)."""
    g = torch.Generator().manual_seed(seed + Hp * 7 + Wp)
    lab = torch.ones(Hp, Wp, dtype=torch.long)
    if pat == "blobs":                                   # smooth random blobs, soft probabilities (as test_trimap_encode)
        sm = F.interpolate(torch.randn(1, 3, max(2, Hp // 64), max(2, Wp // 64), generator=g) * 4, size=(Hp, Wp), mode="bilinear")
        return torch.softmax(sm[0], 0)
    if pat == "corner":                                  # one seed each: distances span the whole diagonal
        lab[0, 0] = 0
        lab[Hp - 1, Wp - 1] = 2
    elif pat == "column_row":                            # bg only in one column (g = EDT_INF elsewhere), fg only in one row
        rows = torch.randperm(Hp, generator=g)[: max(1, Hp // 50)]
        lab[rows, Wp // 3] = 0
        cols = torch.randperm(Wp, generator=g)[: max(1, Wp // 50)]
        lab[(2 * Hp) // 3, cols] = 2
    elif pat == "sparse":                                # ~1e-4 density: typical distances 30-100 px, both sides of the 32-px split
        u = torch.rand(Hp, Wp, generator=g)
        lab[u < 1e-4] = 0
        lab[u > 1 - 1e-4] = 2
        lab[0, Wp // 2] = 0
        lab[Hp - 1, Wp // 2] = 2
    elif pat.startswith("lattice"):                      # seed lattices whose column pitch meets the 32-column coarse blocks
        pb, pf = int(pat.split("_")[1]), int(pat.split("_")[2])
        lab[5::97, 3::pb] = 0
        lab[50::89, 7::pf] = 2
    elif pat == "ties":                                  # pairs of seeds with a band of equidistant pixels between them
        for y in range(Hp // 7, Hp, max(1, Hp // 3)):
            lab[y, max(0, Wp // 2 - 40)] = 0
            lab[y, min(Wp - 1, Wp // 2 + 40)] = 0
        for x in range(Wp // 5, Wp, max(1, Wp // 3)):
            lab[max(0, Hp // 2 - 30), x] = 2
            lab[min(Hp - 1, Hp // 2 + 30), x] = 2
    elif pat == "band":                                  # bg above / fg below a curve, a 1-px unknown band between them
        yy = torch.arange(Hp)[:, None].float()
        xx = torch.arange(Wp)[None, :].float()
        curve = Hp * (0.5 + 0.3 * torch.sin(xx * (6.0 / Wp)))
        lab = torch.where(yy < curve, 0, 2)
        lab[(yy - curve).abs() < 0.5] = 1
    elif pat == "empty":                                 # no fg pixel at all: the fg channels must be zero
        lab[Hp // 3: Hp // 3 + 3, : Wp // 2] = 0
    else:
        raise ValueError(pat)
    return _onehot(lab)


def _encode_full(G, probs):
    """otvm_trimap_encode (as test_gpu_kernels._encode): channels 3..10 of x11, class map, d80[70:72]."""
    from otvm_amd import lib as L
    lib = L.load()
    _, Hp, Wp = probs.shape
    P = Hp * Wp
    pd = probs.contiguous().to(G.DEV)
    x11 = torch.zeros(P * 12, device=G.DEV)
    d80 = torch.zeros(P * 80, device=G.DEV)
    cls = torch.empty(P, dtype=torch.uint8, device=G.DEV)
    ws = torch.empty(int(lib.otvm_trimap_encode_ws_bytes(Hp, Wp)), dtype=torch.uint8, device=G.DEV)
    L.check(lib.otvm_trimap_encode(pd.data_ptr(), Hp, Wp, 0, cls.data_ptr(), x11.data_ptr(), 12, d80.data_ptr(), 80,
                                   ws.data_ptr(), G.stream()))
    torch.cuda.synchronize()
    x = x11.reshape(Hp, Wp, 12)[..., 3:11].permute(2, 0, 1).cpu()
    return x, cls.reshape(Hp, Wp).cpu(), d80.reshape(Hp, Wp, 80)[..., 70:72].cpu()


def _exact_d2(v):
    """Integer squared distance recovered from the sigma = 0.16 channel where it has not underflowed (v > 1e-30, i.e.
    d^2 < ~3.6e5): the rounding of sqrtf, d*d, the division and expf together move -ln(v) * DEN2 by < 0.1 there."""
    v = v.double().numpy()
    ok = v > 1e-30
    d2 = np.full(v.shape, -1, dtype=np.int64)
    d2[ok] = np.rint(-np.log(v[ok]) * DEN2).astype(np.int64)
    return d2, ok


@pytest.mark.parametrize("Hp,Wp,pat", EDT_CASES, ids=lambda v: str(v))
def test_trimap_encode_every_pixel(G, Hp, Wp, pat):
    from scipy import ndimage
    from oracle.otvm_oracle import make_trimap8, class_map
    probs = _edt_probs(Hp, Wp, pat)
    got, cls, tri2 = _encode_full(G, probs)
    cm = class_map(probs)
    assert torch.equal(cls.long(), cm)
    ref = make_trimap8(probs)
    err = G.maxdiff(got, ref)
    assert err <= 2e-6, err
    assert torch.equal(tri2[..., 0], probs[0]) and torch.equal(tri2[..., 1], probs[2])
    report = []
    for k, target in ((0, 0), (1, 2)):
        mask = (cm == target).numpy()
        if not mask.any():
            assert torch.count_nonzero(got[3 * k: 3 * k + 3]) == 0        # empty class -> zeros
            report.append("class %d empty" % target)
            continue
        d = ndimage.distance_transform_edt(~mask)                          # float64 sqrt of the exact integer d^2
        want = np.rint(d * d).astype(np.int64)
        d2, ok = _exact_d2(got[3 * k + 2])
        bad = ok & (d2 != want)
        assert not bad.any(), "class %d: %d pixels with a wrong d^2, first at %s: got %d, want %d" % (
            target, int(bad.sum()), tuple(np.argwhere(bad)[0]), d2[bad][0], want[bad][0])
        assert ok[want < 300000].all()                   # the channel resolves every d^2 below ~3.6e5: all of those were checked
        report.append("class %d: exact d2 on %d px, max d2 checked %d (max d2 %d)" % (target, int(ok.sum()), int(want[ok].max()),
                                                                                     int(want.max())))
    print("edt %dx%d %s: %s; channels max-abs %.2e" % (Hp, Wp, pat, "; ".join(report), err))


# --------------------------------------------------------------------------------------------------- f16x3 memory read
MR_SCALES = [("k0.8", 0.8, 1.0), ("sharp", 16.5, 3.0)]   # key scale (scores ~N(0, 0.5) / span about +-60), dominant-match factor
Q_LD, OUT_LD, OUT_OFF = 136, 528, 8


def _mr_reference(q, keys, vals):
    """softmax over the memory axis of (K q) / sqrt(128), times V, in float64 on the device, in query blocks."""
    K = torch.cat(keys).double()
    V = torch.cat(vals).double()
    out = torch.empty(q.shape[0], 512, dtype=torch.float64, device=q.device)
    step = max(256, (1 << 28) // K.shape[0] // 256 * 256)
    for c0 in range(0, q.shape[0], step):
        s = K @ q[c0:c0 + step].double().t() / math.sqrt(128.0)
        out[c0:c0 + step] = (torch.softmax(s, 0).t() @ V)
    return out


def _mr_inputs(G, hw, T, kscale, dom, seed):
    g = torch.Generator(device=G.DEV).manual_seed(seed)
    q = torch.randn(hw, 128, generator=g, device=G.DEV) * 0.8
    keys = [torch.randn(hw, 128, generator=g, device=G.DEV) * kscale for _ in range(T)]
    vals = [torch.randn(hw, 512, generator=g, device=G.DEV) for _ in range(T)]
    # dominant matches in the last (partially masked) 64-row tile of a slot, i.e. right before the wrap into the next slot,
    # and a still larger one for the same query in the first tile of the next slot: the running max jumps across the wrap
    for t in range(T):
        for j in range(4):
            qi = (977 * (t * 4 + j) + 13) % hw
            keys[t][hw - 1 - j] = q[qi] * (3.0 * dom)
            if t + 1 < T:
                keys[t + 1][j] = q[qi] * (4.0 * dom)
    return q, keys, vals


@pytest.mark.parametrize("scale", MR_SCALES, ids=lambda s: s[0])
@pytest.mark.parametrize("hw,T", MR_SHAPES)
def test_memory_read_chunks_across_slots(G, hw, T, scale):
    from otvm_amd import lib as L
    lib = L.load()
    st = G.stream()
    q, keys, vals = _mr_inputs(G, hw, T, scale[1], scale[2], seed=hw + 31 * T)
    ref = _mr_reference(q, keys, vals)
    bound = 2e-5 * max(1.0, float(ref.abs().max()))
    qbuf = torch.zeros(hw, Q_LD, device=G.DEV)
    qbuf[:, :128] = q
    slots = []
    for t in range(T):
        sl = torch.zeros(int(lib.otvm_bank_slot_bytes_f16x3(hw)), dtype=torch.uint8, device=G.DEV)
        L.check(lib.otvm_bank_pack_f16x3(keys[t].data_ptr(), vals[t].data_ptr(), hw, sl.data_ptr(), st))
        slots.append(sl)
    del keys, vals
    sp = [s_.data_ptr() for s_ in slots]
    outbuf = torch.empty(hw * OUT_LD + OUT_OFF + 16, device=G.DEV)
    out = torch.as_strided(outbuf, (hw, 512), (OUT_LD, 1), OUT_OFF)
    out_ptr = outbuf.data_ptr() + 4 * OUT_OFF
    count = lambda n: int(lib.otvm_memory_read_f16x3_partial_count(n, hw))

    def partial(group, ws, np_cap, part0):
        end = C.c_int(-1)
        L.check(lib.otvm_memory_read_f16x3_partial(qbuf.data_ptr(), Q_LD, (C.c_void_p * len(group))(*group), len(group), hw,
                                                   ws.data_ptr(), np_cap, part0, C.byref(end), st))
        return end.value

    def check(what):
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), what
        err = float((out.double() - ref).abs().max())
        assert err <= bound, "%s: max-abs %.3e > %.3e" % (what, err, bound)
        return err

    # 1. the one-call read
    outbuf.fill_(float("nan"))
    ws = torch.empty(int(lib.otvm_memory_read_ws_bytes(hw, T)), dtype=torch.uint8, device=G.DEV)
    L.check(lib.otvm_memory_read_f16x3(qbuf.data_ptr(), Q_LD, (C.c_void_p * T)(*sp), T, hw, out_ptr, OUT_LD, ws.data_ptr(), st))
    e1 = check("one call")
    del ws
    # 2. the engine's two steps (engine.memory_read_begin / _fresh / _merge): old slots, then the fresh one at part0 = done
    np_cap = count(T - 1) + count(1)
    ws = torch.empty(np_cap * hw * (512 + 2) * 4, dtype=torch.uint8, device=G.DEV)
    done = partial(sp[:-1], ws, np_cap, 0)
    done = partial(sp[-1:], ws, np_cap, done)
    outbuf.fill_(float("nan"))
    L.check(lib.otvm_memory_read_f16x3_combine(ws.data_ptr(), np_cap, done, hw, out_ptr, OUT_LD, st))
    e2 = check("old + fresh")
    del ws
    # 3. one partial launch per slot
    np_cap = T * count(1)
    ws = torch.empty(np_cap * hw * (512 + 2) * 4, dtype=torch.uint8, device=G.DEV)
    done = 0
    for t in range(T):
        done = partial(sp[t:t + 1], ws, np_cap, done)
    outbuf.fill_(float("nan"))
    L.check(lib.otvm_memory_read_f16x3_combine(ws.data_ptr(), np_cap, done, hw, out_ptr, OUT_LD, st))
    e3 = check("singletons")
    # a workspace laid out for one partial too few is refused before anything is launched (ws itself is large enough for
    # np_cap partials, so nothing could land outside it either way)
    end = C.c_int(-1)
    rc = lib.otvm_memory_read_f16x3_partial(qbuf.data_ptr(), Q_LD, (C.c_void_p * T)(*sp), T, hw, ws.data_ptr(), count(T) - 1, 0,
                                            C.byref(end), st)
    assert rc != 0 and end.value == -1 and b"too small" in lib.otvm_last_error()
    torch.cuda.synchronize()
    lau = mr_launches(T, hw)
    print("memread hw=%d T=%d %s: chunk_tiles %s, slot-crossing chunks %s; max-abs one call %.2e, old+fresh %.2e, singletons "
          "%.2e (bound %.2e)" % (hw, T, scale[0], [l["chunk_tiles"] for l in lau], [l["crossing"] for l in lau], e1, e2, e3, bound))


# --------------------------------------------------------------------------------------------------- GroupNorm statistics
GN_SHAPES = [(1088, 1920, 64), (1088, 1920, 256), (136, 240, 2048), (2176, 3840, 64)]
GN_RATIOS = [("r0", 0.0), ("r10", 10.0), ("r100", 100.0), ("r300", 300.0)]    # r300: most groups at 100, four at 300


def _group_offsets(ratio_name, ratio, sigma):
    mu = torch.linspace(-1.0, 1.0, 32, dtype=torch.float64)
    mu = torch.where(mu >= 0, 1.0, -1.0) * sigma
    if ratio_name == "r300":
        r = torch.full((32,), 100.0, dtype=torch.float64)
        r[[0, 9, 17, 31]] = 300.0
    else:
        r = torch.full((32,), ratio, dtype=torch.float64)
    return mu * r


def _moments64(x, C):
    """fp64 two-pass per-group mean / (biased) variance of an NHWC [P, C] tensor, on the device."""
    P = x.shape[0]
    xg = x.reshape(P, 32, C // 32)
    s = torch.zeros(32, dtype=torch.float64, device=x.device)
    step = max(1, (1 << 26) // C)
    for p0 in range(0, P, step):
        s += xg[p0:p0 + step].double().sum((0, 2))
    mean = s / (P * (C // 32))
    v = torch.zeros(32, dtype=torch.float64, device=x.device)
    for p0 in range(0, P, step):
        v += ((xg[p0:p0 + step].double() - mean[None, :, None]) ** 2).sum((0, 2))
    return mean.cpu(), (v / (P * (C // 32))).cpu()


def _moments_cpu32(xt, C):
    """the fp32 CPU evaluation the bound is measured against: torch.var_mean per group of the fp32 tensor, given as a [C, P] CPU
    tensor (channel-major: a group's values are one contiguous run)."""
    xc = xt.reshape(32, -1)
    var, mean = torch.var_mean(xc, 1, unbiased=False)
    return mean.double(), var.double()


def _stats_moments(stats, P, C):
    """mean / variance as every consumer derives them from the fp64 sums (gn_apply_kernel, gn_table_kernel)."""
    s = stats.cpu().reshape(32, 2)
    cnt = float(P * (C // 32))
    mean = s[:, 0] / cnt
    return mean, s[:, 1] / cnt - mean * mean


def _moment_errors(mean, var, mean64, var64):
    sd = var64.sqrt()
    return float(((mean - mean64).abs() / sd).max()), float(((var - var64).abs() / var64).max())


def _check_moments(what, dev, cpu, ref):
    em_d, ev_d = _moment_errors(*dev, *ref)
    em_c, ev_c = _moment_errors(*cpu, *ref)
    print("%s: mean err / sd: device %.2e, torch fp32 %.2e; var rel err: device %.2e, torch fp32 %.2e" % (what, em_d, em_c, ev_d, ev_c))
    assert em_d <= max(1e-6, 2 * em_c), (what, em_d, em_c)
    assert ev_d <= max(1e-6, 2 * ev_c), (what, ev_d, ev_c)


@pytest.mark.parametrize("ratio", GN_RATIOS, ids=lambda r: r[0])
@pytest.mark.parametrize("H,W,Cc", GN_SHAPES)
def test_groupnorm_statistics_full_resolution(G, H, W, Cc, ratio):
    """x = mu_g + sigma z with |mu_g| / sigma = ratio: the device's fp64 sums must give the two-pass fp64 mean / variance within
    1e-6 (mean relative to the group's sd, variance relative), or no worse than 2x a torch fp32 CPU evaluation; the apply output
    must meet the same comparative bound against fp64 GroupNorm, measured with torch's fp32 CPU F.group_norm."""
    from otvm_amd import lib as L
    lib = L.load()
    P = H * W
    g = torch.Generator(device=G.DEV).manual_seed(P + Cc)
    sigma = 0.7
    mu = _group_offsets(ratio[0], ratio[1], sigma).float().to(G.DEV)
    x = torch.randn(P, 32, Cc // 32, generator=g, device=G.DEV) * sigma + mu[None, :, None]
    x = x.reshape(P, Cc).contiguous()
    stats = torch.zeros(64, dtype=torch.float64, device=G.DEV)
    L.check(lib.otvm_gn_stats(x.data_ptr(), P, Cc, Cc, stats.data_ptr(), G.stream()))
    torch.cuda.synchronize()
    ref = _moments64(x, Cc)
    xt = x.t().contiguous().cpu()                        # the one host copy: [C, P], the layout F.group_norm takes
    _check_moments("gn_stats %dx%dx%d %s" % (H, W, Cc, ratio[0]), _stats_moments(stats, P, Cc), _moments_cpu32(xt, Cc), ref)

    gc = torch.Generator().manual_seed(7)
    gamma, beta = torch.randn(Cc, generator=gc) + 1, torch.randn(Cc, generator=gc)
    out = torch.empty_like(x)
    gd, bd = gamma.to(G.DEV), beta.to(G.DEV)
    L.check(lib.otvm_gn_apply(x.data_ptr(), P, Cc, Cc, stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), 0, 0, 0, 0, 0, 0,
                              out.data_ptr(), Cc, G.stream()))
    torch.cuda.synchronize()
    # fp64 GroupNorm from the fp64 moments (on the device); torch fp32 CPU GroupNorm on [1, C, P]
    m64, v64 = ref[0].to(G.DEV), ref[1].to(G.DEV)
    rs = (v64 + 1e-5).rsqrt()
    a64 = (rs.repeat_interleave(Cc // 32) * gd.double())
    b64 = bd.double() - m64.repeat_interleave(Cc // 32) * a64
    err_d = err_c = 0.0
    cpu = F.group_norm(xt[None], 32, gamma, beta, 1e-5)[0]
    del xt
    step = max(1, (1 << 26) // Cc)
    for p0 in range(0, P, step):
        y64 = x[p0:p0 + step].double() * a64 + b64
        err_d = max(err_d, float((out[p0:p0 + step].double() - y64).abs().max()))
        err_c = max(err_c, float((cpu[:, p0:p0 + step].to(G.DEV).t().double() - y64).abs().max()))
    print("gn_apply %dx%dx%d %s: max-abs vs fp64: device %.2e, torch fp32 %.2e" % (H, W, Cc, ratio[0], err_d, err_c))
    assert err_d <= max(1e-6, 2 * err_c), (err_d, err_c)


@pytest.mark.parametrize("ratio", [("r0", 0.0), ("r100", 100.0)], ids=lambda r: r[0])
def test_conv_fused_groupnorm_statistics_full_resolution(G, ratio):
    """The conv epilogue's GroupNorm sums (otvm_conv_params.gn_stats) of a 1088x1920 64->64 3x3 conv with a bias of ratio x the
    output's sd per group, against fp64 two-pass moments of the output the kernel itself wrote (conv error stays out)."""
    H, W, Cin, Cout = 1088, 1920, 64, 64
    g = torch.Generator().manual_seed(91)
    x = torch.randn(1, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = (_group_offsets(ratio[0], ratio[1], 1.0).repeat_interleave(Cout // 32) + 0.05 * torch.randn(Cout, generator=g, dtype=torch.float64)).float()
    out = G.empty_act(H, W, Cout)
    stats = torch.zeros(64, dtype=torch.float64, device=G.DEV)
    G.conv2d(G.to_act(x), G.pack_weight(w), out, bias.to(G.DEV), pad=1, precision=1, gn_stats=stats)
    y = torch.as_strided(out.t, (H * W, Cout), (out.ld, 1), out.off)
    assert torch.isfinite(y).all()
    _check_moments("conv gn_stats %dx%d %d->%d %s" % (H, W, Cin, Cout, ratio[0]), _stats_moments(stats, H * W, Cout),
                   _moments_cpu32(y.t().contiguous().cpu(), Cout), _moments64(y, Cout))
