"""Reference composition for keyframe clips (TEST INFRASTRUCTURE: imports the CPU oracle; never on the product path).

The reference model takes a trimap on a clip's first frame only (models/alpha/model.py:425-443), so there is nothing in it to
run a mid-clip keyframe against.  What it does have are the stages: this file composes OtvmOracle's OWN ``stm_segment``,
``make_trimap8``, ``fba``, ``stm_memorize`` and padding -- the functions the rest of the suite pins against
reference-generated fixtures -- under the keyframe schedule, with the anchor policy and the schedule restated here
independently of ``otvm_amd.engine.bank_update`` and ``otvm_amd.video.keyframe_schedule``.

  full keyframe : the padded trimap is the network's trimap input (as on a first frame); no segment; the bank is kept
  correction    : softmax of the segment's logits, then the exact one-hot of the label wherever the map has one
  anchor policy : a slot of a frame that was given a trimap never leaves; one more slot of room per extra anchor
"""
import torch
import torch.nn.functional as F

from oracle.otvm_oracle import OtvmOracle, class_map, make_trimap8, pad_amounts


class Slot:
    __slots__ = ("k", "v", "frame", "anchor")

    def __init__(self, k, v, frame, anchor):
        self.k, self.v, self.frame, self.anchor = k, v, frame, anchor


def anchor_policy(bank, new, first_frame, memorize, max_memory_num):
    """The bank after ``new`` (a Slot carrying its own anchor flag) was memorised; max_memory_num >= 2."""
    assert max_memory_num >= 2
    if first_frame:
        return [new]
    grows = new.anchor or memorize or len(bank) == 1 or bank[-1].anchor
    bank = list(bank) + [new] if grows else list(bank[:-1]) + [new]
    room = max_memory_num + sum(1 for s in bank if s.anchor) - 1
    while len(bank) > room:
        del bank[[i for i, s in enumerate(bank) if not s.anchor][0]]
    return bank


def schedule(T, kinds, skip):
    """kinds: {frame: "key" | "labels"}.  Steps (t, kind, first_frame, last_frame, memorize) in the order they are matted."""
    keys = sorted(t for t, k in kinds.items() if k == "key")
    k0 = keys[0]
    order = list(keys)
    order += [t for t in range(k0 + 1, T) if t not in keys]
    order += list(range(k0 - 1, -1, -1))
    steps = []
    for n, t in enumerate(order):
        memorize = skip > 2 and abs(t - k0) % skip == 0
        steps.append((t, kinds.get(t, "frame"), t == k0, n == len(order) - 1, memorize))
    return steps


class KeyframeComposition:
    """Steps a demo-flow clip (a = 1, bg = fg) through the oracle's stages."""

    def __init__(self, state_dict, dilate_kernel=12, read_dtype=None):
        self.orc = OtvmOracle(state_dict, dilate_kernel=dilate_kernel, read_dtype=read_dtype)
        self.bank = []

    def frames(self):
        return [s.frame for s in self.bank]

    def anchors(self):
        return [s.frame for s in self.bank if s.anchor]

    def drop_non_anchors(self):
        self.bank = [s for s in self.bank if s.anchor]

    def step(self, fg, t, kind, first_frame, last_frame, memorize, max_memory_num, tri=None, labels=None, cls_hip=None):
        """fg [1,3,H,W] BGR 0..255 float; tri one-hot [3,H,W] (first frame / full keyframe); labels uint8 [H,W] (correction).
        cls_hip: the class map the device path used ([Hp,Wp] long) -- the suite's tie-break protocol: where it differs from the
        composition's own argmax every differing pixel must be a near-tie (top-2 gap < 2e-3), and the composition goes on with
        the device's tie-breaks.  Returns dict(alpha [H,W], T_read, ties, cls [Hp,Wp], tri_in [3,Hp,Wp])."""
        orc = self.orc
        dt = orc.dtype
        a4 = torch.ones(1, 1, fg.shape[-2], fg.shape[-1], dtype=dt)
        f4 = fg.to(dt).flip([1]) * (1.0 / 255)
        img = f4 * a4 + f4 * (1.0 - a4)
        H, W = img.shape[-2:]
        pad = pad_amounts(H, W, 32)
        lw, uw, lh, uh = pad
        imgp = F.pad(img, pad) if sum(pad) else img
        imgn = (imgp - orc.mean) / orc.std
        T_read = 0
        if first_frame or kind == "key":
            t3 = torch.as_tensor(tri).to(dt)[None]
            tri_in = torch.cat((F.pad(t3[:, :1], pad, value=1.0), F.pad(t3[:, 1:], pad, value=0.0)), 1) if sum(pad) else t3
        else:
            T_read = len(self.bank)
            logits = orc.stm_segment(imgp, [(s.k, s.v) for s in self.bank])
            tri_in = F.softmax(logits, dim=1)
            if kind == "labels":
                lab = torch.as_tensor(labels).long()
                has = lab != 255
                onehot = F.one_hot(lab.clamp(max=2), 3).permute(2, 0, 1).to(dt)
                inner = tri_in[0, :, lh:lh + H, lw:lw + W]
                tri_in[0, :, lh:lh + H, lw:lw + W] = torch.where(has[None], onehot, inner)
        cls = class_map(tri_in[0])
        ties = 0
        if cls_hip is not None and not torch.equal(cls_hip, cls):
            diff = cls_hip != cls
            ties = int(diff.sum())
            top2 = torch.sort(tri_in[0], dim=0, descending=True)[0]
            gap = float((top2[0] - top2[1])[diff].max())
            assert gap < 2e-3, "frame %d: class map differs at a pixel that is not a near-tie (gap %g)" % (t, gap)
            cls = cls_hip
        tri8 = make_trimap8(tri_in[0], cls)[None]
        x11 = torch.cat([imgn, tri8], dim=1)
        _, hid, ref7, tri_logits = orc.fba(x11, imgp, tri8[:, -2:])
        alpha = ref7[:, :1]
        tri_out = F.softmax(tri_logits, dim=1)
        if first_frame:
            self.bank = []
        if not last_frame:
            k, v = orc.stm_memorize(imgp, tri_out, alpha, hid)
            new = Slot(k, v, t, first_frame or kind == "key")
            self.bank = anchor_policy(self.bank, new, first_frame, memorize, max_memory_num)
        Hp, Wp = imgp.shape[-2:]
        return dict(alpha=alpha[0, 0, lh:Hp - uh, lw:Wp - uw], T_read=T_read, ties=ties, cls=cls, tri_in=tri_in[0])
