"""Mirror of reference ``models/alpha/model.py::EvalModel`` (lines 314-512): THE drop-in boundary.

Same constructor (``dilate_kernel, trimap, stage``), same 785-key ``state_dict``, same stateful
``forward(a, fg, bg, tri=None, tri_gt=None, first_frame=False, last_frame=False, memorize=False,
max_memory_num=2, large_input=False)`` returning the same 5-tuple.  All device work goes through
``libotvm_hip.so``; there is no PyTorch/CPU fallback -- on a CPU device ``forward`` raises.
"""
import numpy as np
import torch
from torch import nn

from .engine import HipEngine
from .modules import attach_from_spec


def background_colour(bg, who="otvm_amd"):
    """The rule for a colour to composite over: three values in 0..255 (``who`` names the caller in the refusal)."""
    c = tuple(int(x) for x in bg)
    if len(c) != 3 or not all(0 <= x <= 255 for x in c):
        raise ValueError("%s: a background colour is three values in 0..255, got %r" % (who, bg))
    return c


class EvalModel(nn.Module):
    def __init__(self, dilate_kernel=None, eps=0, trimap=None, stage=1):
        super().__init__()
        if stage != 4 or trimap is None:
            raise NotImplementedError("otvm_amd implements the stage-4 (joint trimap+alpha) inference path only")
        self.stage = stage
        self.refinement = True
        self.DILATION_KERNEL = dilate_kernel
        self.EPS = eps
        self.IMG_SCALE = 1.0 / 255
        self.TRIMAP_CHANNEL = 8
        self.memory_update = False
        attach_from_spec(self, "", "")           # everything except the trimap.* keys ...
        for k in [k for k in self._modules if k == "trimap"]:
            del self._modules[k]
        self.trimap = trimap                      # ... which live in the FullModel_eval passed in (alpha/model.py:37)
        self._engine = None
        self._engine_key = None
        self.precision = None                     # None -> OTVM_PRECISION env or "f16x3"; "f32" = exact-fp32 MFMA
        # extension (not part of the reference surface): keep the refinement head's foreground estimate F and publish, per
        # frame, engine.last_fgr ([3,H,W] fp32 RGB), last_rgba_u8 ([H,W,4]) and, with set_background, last_comp_u8 ([H,W,3]).
        # Read at a clip's first frame; forward's signature and 5-tuple do not change.
        self.foreground = False
        self._background = None

    # -- engine lifetime: rebuilt when the weights change or the module moves
    def _get_engine(self):
        dev = self.IMG_MEAN.device
        if dev.type != "cuda":
            raise RuntimeError("otvm_amd.EvalModel: parameters are on %s; move the model to the GPU (.cuda()) -- "
                               "the HIP path has no CPU fallback" % dev)
        key = (str(dev), self.precision, tuple(p._version for p in self.parameters()),
               tuple(b._version for b in self.buffers()))
        if self._engine is None or key != self._engine_key:
            self._engine = HipEngine(self.state_dict(), dev, precision=self.precision)
            self._engine_key = key
        return self._engine

    def set_background(self, bg):
        """What ``last_comp_u8`` is composited over (``foreground`` on): None = no composite; a TUPLE (c0, c1, c2) = a colour; a
        uint8 [H,W,3] tensor / array = an image of the frames' resolution; a LIST = one of those per sequence of
        ``forward_batch``.  Colours and images are in the frames' channel order (B, G, R unless the frames are RGB).  May
        change between frames."""
        self._background = [self._one_background(x) for x in bg] if isinstance(bg, list) else self._one_background(bg)

    def _one_background(self, bg):
        if bg is None:
            return None
        if isinstance(bg, tuple):
            return background_colour(bg)
        t = bg if torch.is_tensor(bg) else torch.from_numpy(np.ascontiguousarray(bg))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError("otvm_amd: a background image is uint8 [H,W,3], got %s %s" % (t.dtype, tuple(t.shape)))
        return t.to(self.IMG_MEAN.device).contiguous()

    def _push_options(self, eng):
        eng.foreground = bool(self.foreground)
        eng.background = self._background

    @property
    def memories(self):
        """Bank introspection (reference: self.memories['key'].shape[3] slots): the frame ids resident, and those of them
        that are anchors (frames that were given a trimap: the first frame, keyframes)."""
        eng = self._engine
        if eng is None:
            return {"frames": [], "anchors": []}
        return {"frames": eng.bank_frames(), "anchors": eng.bank_anchors()}

    def drop_non_anchors(self):
        """Keep only the anchor slots of the memory bank (video.run_video_matte: before the backward sweep of a keyframe clip)."""
        if self._engine is not None:
            self._engine.drop_non_anchors()

    def drop_plans(self):
        """Forget every frame plan of the engine, with its buffers and the memory bank (a process that mattes clips of many sizes
        -- a region-of-interest window per clip -- calls this BETWEEN clips; the next frame plans again)."""
        if self._engine is not None:
            self._engine._drop_plans()

    @torch.no_grad()
    def forward(self, a, fg, bg, tri=None, tri_gt=None, first_frame=False, last_frame=False, memorize=False,
                max_memory_num=2, large_input=False, keyframe=False, labels=None, _frame_id=None, _cls_override=None,
                _frames_rgb=False, _inputs_ready=None):
        """Extensions behind the reference's arguments (defaults = the reference's frame step):
        keyframe=True with ``tri_gt`` on a later frame: the frame runs on that trimap as a first frame does -- no propagation, no
        memory read -- WITHOUT resetting the bank, and is memorised as an anchor slot, which the bank policy never evicts;
        labels = uint8 [H,W] (0 bg, 1 unknown, 2 fg, 255 unlabelled) on a later frame: the propagated trimap is overwritten with
        the exact one-hot of the label wherever there is one (keyframe=True then only makes the slot an anchor).
        Both need max_memory_num >= 2; neither exists for forward_batch."""
        if tri is not None:
            # alpha/model.py:395-396: unreachable from eval.py (EvalDataset is built with trimap=None, eval.py:133); a trimap for
            # a later frame goes through tri_gt with keyframe=True
            raise NotImplementedError("per-frame `tri` input is not part of the reference eval path (a later frame's trimap: "
                                      "tri_gt with keyframe=True)")
        eng = self._get_engine()
        self._push_options(eng)
        out = eng.frame(a, fg, bg, tri_gt=tri_gt, first_frame=bool(first_frame), last_frame=bool(last_frame),
                        memorize=bool(memorize), max_memory_num=int(max_memory_num),
                        dilate_kernel=self.DILATION_KERNEL, frame_id=_frame_id, cls_override=_cls_override,
                        frames_rgb=bool(_frames_rgb), inputs_ready=_inputs_ready, keyframe=bool(keyframe), labels=labels)
        self.memory_update = memorize
        return out

    @torch.no_grad()
    def forward_batch(self, a, fg, bg, tri_gt, first_frame=False, last_frame=False, memorize=False, max_memory_num=2,
                      large_input=False, _frames_rgb=False, _inputs_ready=None, _cls_override=None, keyframe=False, labels=None):
        """Round 3 extension (not part of the reference surface): the same frame step for B independent sequences stepped in
        LOCK-STEP -- ``a``, ``fg``, ``bg``, ``tri_gt`` are lists of B per-sequence inputs shaped as ``forward`` takes them
        (one resolution, one memory schedule; every sequence keeps its own memory bank).  Every layer runs as one launch
        over the B images, which fills the chip on the small maps a single sequence leaves mostly idle.  Returns a list of
        B 5-tuples; each equals what ``forward`` returns for that sequence run alone with the same kernel configurations."""
        if keyframe or labels is not None:
            raise NotImplementedError("otvm_amd: keyframe / labels are single-sequence options of forward()")
        eng = self._get_engine()
        self._push_options(eng)
        out = eng.frame_batch(list(a), list(fg), list(bg), list(tri_gt), first_frame=bool(first_frame), last_frame=bool(last_frame),
                              memorize=bool(memorize), max_memory_num=int(max_memory_num), dilate_kernel=self.DILATION_KERNEL,
                              cls_override=_cls_override, frames_rgb=bool(_frames_rgb), inputs_ready=_inputs_ready)
        self.memory_update = memorize
        return out


class FullModel(EvalModel):
    """Mirror of the reference's TRAINING class ``models/alpha/model.py::FullModel`` (lines 9-312), forward only: same
    constructor and state_dict as ``EvalModel``, ``forward(a, fg, bg, ignore_region=None, tri=None)`` over a batch of clips
    ``[B, S, C, H, W]`` returning the reference's list ``[loss1, loss2, loss3, loss_trimap, scaled_imgs, tris_vis, alphas, comps,
    scaled_gts, Fs, Bs, preds_trimap]`` (otvm_amd/train.py).  There is no backward: the library holds no gradient kernels."""
    FBA_LOSS_NORMALIZE = True

    @torch.no_grad()
    def forward(self, a, fg, bg, ignore_region=None, tri=None):
        if ignore_region is not None:
            raise NotImplementedError("ignore_region is not used by the stage-4 training loop of the reference")
        from .train import train_forward
        return train_forward(self, a, fg, bg, tri)
