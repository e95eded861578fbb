"""Every accumulator of the training-loss kernels (csrc/losses.hip) on its own, restated with torch on the CPU on top of the
functions of oracle/train_oracle.py (which tests/golden/train_*.npz pin to the reference).  No GPU import.

Each function takes ``dt``:
  torch.float64 -- the reference: float64 throughout;
  torch.float32 -- the yardstick: every element computed in float32 by torch's own statements (an arithmetic that owes nothing to
                   the kernels), every sum taken in float64.  How far it lies from the reference is what float32 elements cost.
Sums come back as Python floats / float64 tensors, elementwise tensors in ``dt``.  ``loss_from_terms`` puts the sums together with
the weights of otvm_amd/train.py::_fba_loss; tests/test_glue_train_cpu.py shows that this is train_oracle.fba_loss."""
import torch
import torch.nn.functional as F

from oracle import train_oracle as T

EPS = 1.001e-5
f64 = torch.float64


def _sum(x):
    return float(x.to(f64).sum())


def fba_comp(pred7, gts, tm, fgs, bgs, imgs, dt=f64):
    """pred7 [B,S,7,H,W]; gts, tm [B,S,1,H,W]; fgs, bgs, imgs [B,S,3,H,W] -> dict(sums[5], alphas, Fs, Bs, comps)."""
    pred7, gts, tm, fgs, bgs, imgs = (x.to(dt) for x in (pred7, gts, tm, fgs, bgs, imgs))
    a = pred7[:, :, :1]
    m = tm != 0
    cF = torch.where((m & (gts > 0)).expand_as(fgs), pred7[:, :, 1:4], fgs)          # train_oracle.fba_loss, the same statements
    cB = torch.where(m.expand_as(bgs), pred7[:, :, 4:7], bgs)
    comp = cF * a + cB * (1. - a)
    sums = [_sum(torch.abs(a - gts)), _sum(torch.abs(cF * gts + cB * (1. - gts) - imgs)),
            _sum(torch.abs(fgs * a + bgs * (1. - a) - imgs)), _sum(torch.abs(cF - fgs)), _sum(torch.abs(cB - bgs))]
    return dict(sums=sums, alphas=a.contiguous(), Fs=cF, Bs=cB, comps=comp)


def grad_l1(x, y, dt=f64):
    """x, y [N,H,W] -> sum | sqrt(gx^2 + gy^2 + eps)(x) - same(y) |  (train_oracle.l1_grad without the mean)."""
    fx, fy = T.get_gradient(x.to(dt)[:, None])
    tx, ty = T.get_gradient(y.to(dt)[:, None])
    return _sum(torch.abs(torch.sqrt(fx ** 2 + fy ** 2 + EPS) - torch.sqrt(tx ** 2 + ty ** 2 + EPS)))


def exclusion_level(i1, i2, dt=f64):
    """i1, i2 [B,S,3,H,W] -> acc1 [S,4] = per frame sum |gx1|, |gy1|, |gx2|, |gy2| over the batch; acc2 [B*S,2] = per (b, frame) sum
    of (2 sig(gx1) - 1)^2 (2 sig(gx2 alphax) - 1)^2 and the same in y  (train_oracle.exclusion_loss, one level, frame by frame)."""
    i1, i2 = i1.to(dt), i2.to(dt)
    B, S = i1.shape[:2]
    acc1 = torch.zeros(S, 4, dtype=f64)
    acc2 = torch.zeros(B * S, 2, dtype=f64)
    for c in range(S):
        gx1, gy1 = T.get_gradient(i1[:, c])
        gx2, gy2 = T.get_gradient(i2[:, c])
        for k, g in enumerate((gx1, gy1, gx2, gy2)):
            acc1[c, k] = torch.abs(g).to(f64).sum()
        mean = (acc1[c] / float(gx1.numel())).to(dt)                                # the means from the float64 sums
        ax = 2.0 * mean[0] / (mean[2] + EPS)
        ay = 2.0 * mean[1] / (mean[3] + EPS)
        gx1s, gy1s = torch.sigmoid(gx1) * 2 - 1, torch.sigmoid(gy1) * 2 - 1
        gx2s, gy2s = torch.sigmoid(gx2 * ax) * 2 - 1, torch.sigmoid(gy2 * ay) * 2 - 1
        for b in range(B):
            acc2[b * S + c, 0] = ((gx1s[b] ** 2) * (gx2s[b] ** 2)).to(f64).sum()
            acc2[b * S + c, 1] = ((gy1s[b] ** 2) * (gy2s[b] ** 2)).to(f64).sum()
    return acc1, acc2


def avgpool2(x, dt=f64):
    """x [N,H,W] -> [N,H/2,W/2]: F.avg_pool2d(x, 2, 2) with the four adds in row-major order, then * 0.25."""
    x = x.to(dt)
    return (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) * 0.25


def lap_level(cur_i, cur_t, weight, dt=f64):
    """cur_i, cur_t [N,H,W] -> (weight * sum |(cur_i - up(down_i)) - (cur_t - up(down_t))|, down_i, down_t): one level of
    train_oracle.laplacian_pyramid for the image and the target."""
    k = T.GAUSS.to(dt)[None, None]
    out = []
    for cur in (cur_i, cur_t):
        cur = cur.to(dt)[:, None]
        down = T._conv_gauss(cur, k)[:, :, ::2, ::2]
        out.append((cur - T._lap_up(down, k), down[:, 0].contiguous()))
    return float(weight) * _sum(torch.abs(out[0][0] - out[1][0])), out[0][1], out[1][1]


def temporal(x, y, dt=f64):
    """x, y [B,S,C,H,W] -> sum ((x[t+1] - x[t]) - (y[t+1] - y[t]))^2."""
    x, y = x.to(dt), y.to(dt)
    d = (x[:, 1:] - x[:, :-1]) - (y[:, 1:] - y[:, :-1])
    return float((d.to(f64) ** 2).sum())


def ce3(lg, cls, dt=f64):
    """lg [N,3,H,W], cls [N,H,W] integer -> sum of -log_softmax(lg)[cls]."""
    return _sum(F.cross_entropy(lg.to(dt), cls.long(), reduction="none"))


def all_terms(pred7, gts, tm, fgs, bgs, imgs, dt=f64):
    """Every accumulator _fba_loss fills, in its slots' order: comp[5], grad, excl = [(acc1, acc2) x 3 levels], lap[3], temp[3]."""
    B, S, _, H, W = pred7.shape
    N = B * S
    fc = fba_comp(pred7, gts, tm, fgs, bgs, imgs, dt)
    al, cF, cB = fc["alphas"], fc["Fs"], fc["Bs"]
    gts, fgs, bgs = gts.to(dt), fgs.to(dt), bgs.to(dt)
    out = dict(comp=fc["sums"], grad=grad_l1(al.reshape(N, H, W), gts.reshape(N, H, W), dt), excl=[], lap=[], temp=[],
               alphas=al, Fs=cF, Bs=cB, comps=fc["comps"])
    i1, i2, h, w = cF, cB, H, W
    for lv in range(3):
        out["excl"].append(exclusion_level(i1, i2, dt))
        if lv < 2:
            i1 = avgpool2(i1.reshape(N * 3, h, w), dt).reshape(B, S, 3, h // 2, w // 2)
            i2 = avgpool2(i2.reshape(N * 3, h, w), dt).reshape(B, S, 3, h // 2, w // 2)
            h, w = h // 2, w // 2
    for x, y, n in ((al, gts, N), (cF, fgs, N * 3), (cB, bgs, N * 3)):
        ci, ct, tot = x.reshape(n, H, W), y.reshape(n, H, W), 0.0
        for lv in range(5):
            s, ci, ct = lap_level(ci, ct, 2 ** lv, dt)
            tot += s
        out["lap"].append(tot)
        out["temp"].append(temporal(x, y, dt) if S > 1 else 0.0)
    return out


def loss_from_terms(t, B, S, H, W):
    """(L_alpha_comp, L_lap, L_grad) with the weights and counts of otvm_amd/train.py::_fba_loss."""
    N, P = B * S, H * W
    c1, c3 = float(N * P), float(N * 3 * P)
    v = t["comp"]
    L_ac = v[0] / c1 + v[1] / c3 + 0.25 * (v[2] / c3 + v[3] / c3 + v[4] / c3)
    excl, h, w = 0.0, H, W
    for _, acc2 in t["excl"]:
        excl += float(((acc2 / (3.0 * h * w) + EPS) ** 0.25).sum())
        h, w = h // 2, w // 2
    excl /= float(B * 3 * S)
    L_grad = t["grad"] / c1 + 0.25 * excl
    L_lap = t["lap"][0] / c1 + 0.25 * (t["lap"][1] / c3 + t["lap"][2] / c3)
    if S > 1:
        t1, t3 = float(B * (S - 1) * P), float(B * (S - 1) * 3 * P)
        L_grad += t["temp"][0] / t1 + 0.25 * (t["temp"][1] / t3 + t["temp"][2] / t3)
    return L_ac, L_lap, L_grad


def rel(got, want):
    """max relative distance of sums (scalars or tensors), with the zero sums that an identically-zero gradient gives compared
    absolutely: |got - want| / max(|want|, tiny)."""
    got, want = torch.as_tensor(got, dtype=f64), torch.as_tensor(want, dtype=f64)
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) if want.numel() else 0.0
