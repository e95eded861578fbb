"""GPU (-m gpu): multi-subject matting.  otvm_subjects_track / _crop / _bbox against S calls of the single-subject kernels
(otvm_roi_track, otvm_roi_crop_at, otvm_trimap_bbox), otvm_subjects_resolve against S otvm_roi_paste_at calls (normalise = 0) and
against its restatement (tests/subjects_ref.py), every comparison bit for bit; run_video_matte_subjects and eval_cli --subjects
against run_video_matte of every subject alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mask_trimap_ref as MR
from tests import roi_ref as R
from tests import subjects_ref as SR
from tests.test_gpu_roi import _frame_inputs, _window_results, bits, dev, stream
from tests.test_gpu_roi_track import _crop_at_raw, _paste_at_raw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5A5A5A5A
# (H, W, h, w): the scalar path (no side a multiple of four), and the vector path
SHAPES = [(37, 53, 16, 20), (64, 96, 32, 32)]
IDS = ["37x53/16x20", "64x96/32x32"]
COUNTS = (1, 3, 8)
PLANES = ("alpha", "alpha_u8", "trimap", "fgr")
ALL = PLANES + ("union", "union_u8", "owner")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from otvm_amd import lib as L
    return L.load()


def _origins(S, H, W, h, w):
    """What the log may hold: the four corners, two equal origins, and stale rows -- negative and too large, which the kernels
    clamp.  S = 1 takes the too-large row, S = 3 the two equal ones and the negative row, S = 8 all."""
    rows = [(0, 0), (0, W - w), (H - h, 0), (H - h, W - w), (3, 5), (3, 5), (-4, -9), (H + 2, W - w + 1)]
    return {1: rows[7:], 3: rows[4:7], 8: rows}[S]


def _log(origins, fill=JUNK):
    """An int32 [S,T=2,10] log on the device, junk everywhere but words 8, 9 of frame 1: the kernels get strided views of it."""
    log = torch.full((len(origins), 2, 10), fill, dtype=torch.int32, device=DEV)
    log[:, 1, 8:] = dev(np.array(origins, np.int32))
    return log


def _offset(shape, dtype, fill, off):
    """A tensor of ``shape`` that starts ``off`` elements into its allocation (off = 1: a base that is not 16-byte -- for bytes not
    4-byte -- aligned), pre-filled with junk."""
    n = int(np.prod(shape))
    return torch.full((n + off,), fill, dtype=dtype, device=DEV)[off:].view(shape)


def _shifted(x, off):
    t = _offset(tuple(x.shape), x.dtype, 0, off)
    t.copy_(x)
    return t


# ------------------------------------------------------------------------------------------------ track
def _track_raw(lib, box, prev, out, H, W, h, w, hold, over=None):
    from otvm_amd import lib as L
    p = L.SubjectsTrackParams()
    p.S, p.H, p.W, p.h, p.w, p.hold = out.shape[0], H, W, h, w, hold
    p.box_base, p.box_stride = box.data_ptr(), box.stride(0)
    if prev is not None:
        p.prev_base, p.prev_stride = prev.data_ptr(), prev.stride(0)
    p.out_base, p.out_stride = out.data_ptr(), out.stride(0)
    for k, v in (over or {}).items():
        setattr(p, k, v)
    rc = lib.otvm_subjects_track(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("S", COUNTS)
@pytest.mark.parametrize("H,W,h,w", SHAPES, ids=IDS)
def test_track_equals_s_single_subject_calls(lib, H, W, h, w, S):
    from otvm_amd import roi, subjects
    g = np.random.default_rng(100 * S + H)
    for hold in (1, 4):
        for with_prev in (True, False):
            sh, sw = (h, w) if with_prev else (H, W)                       # the space the boxes live in
            boxes = []
            for s in range(S):
                y0, x0 = int(g.integers(0, sh)), int(g.integers(0, sw))
                boxes.append((7, 7, 3, 3, y0, x0, int(g.integers(y0, sh)), int(g.integers(x0, sw))))
            boxes[0] = (7, 7, 3, 3, sh, sw, -1, -1)                        # an empty box
            if S > 1:
                boxes[1] = (7, 7, 3, 3, 0, 0, sh - 1, sw - 1)              # a box that touches every side
            log = _log(_origins(S, H, W, h, w))
            log[:, 0, :8] = dev(np.array(boxes, np.int32))
            log[:, 0, 8:] = log[:, 1, 8:]                                  # frame 0's origins: the stale rows among them
            log[:, 1, 8:] = JUNK
            want = torch.full((S, 2), JUNK, dtype=torch.int32, device=DEV)
            for s in range(S):
                roi.track(log[s, 0, :8], log[s, 0, 8:] if with_prev else None, want[s], (h, w), H, W, hold)
            before = log.clone()
            subjects.track(log[:, 0, :8], log[:, 0, 8:] if with_prev else None, log[:, 1, 8:], (h, w), H, W, hold)
            torch.cuda.synchronize()
            assert torch.equal(log[:, 1, 8:], want), (hold, with_prev, log[:, 1, 8:].tolist(), want.tolist())
            assert (want[:, 0] >= 0).all() and (want[:, 0] <= H - h).all() and (want[:, 1] >= 0).all() and (want[:, 1] <= W - w).all()
            assert torch.equal(log[:, 0], before[:, 0]) and torch.equal(log[:, 1, :8], before[:, 1, :8])   # nothing else is written
            # the host policy says the same (boxes in frame coordinates there)
            for s in range(S):
                b, prev = boxes[s][4:], None
                if with_prev:
                    prev = SR.clamp_origin(before[s, 0, 8:].tolist(), (h, w), H, W)
                    b = b if roi.is_empty(b) else (b[0] + prev[0], b[1] + prev[1], b[2] + prev[0], b[3] + prev[1])
                assert tuple(want[s].tolist()) == roi.track_origin(b, prev, h, w, H, W, hold)


# ------------------------------------------------------------------------------------------------ crop
def _crop_raw(lib, origins, H, W, h, w, frame, trimaps, off=0, over=None):
    """One otvm_subjects_crop call on outputs pre-filled with junk -> (rc, [frame windows] or None, [trimap windows] or None)"""
    from otvm_amd import lib as L
    S = origins.shape[0]
    p = L.SubjectsCropParams()
    p.S, p.H, p.W, p.h, p.w = S, H, W, h, w
    p.origin_base, p.origin_stride = origins.data_ptr(), origins.stride(0)
    fo = to = None
    if frame is not None:
        p.frame = frame.data_ptr()
        fo = [_offset((h, w, 3), torch.uint8, 77, off) for _ in range(S)]
    if trimaps is not None:
        to = [_offset((3, h, w), torch.float32, -7.0, off) for _ in range(S)]
    for s in range(S):
        if fo is not None:
            p.frame_out[s] = fo[s].data_ptr()
        if to is not None:
            p.trimap[s], p.trimap_out[s] = trimaps[s].data_ptr(), to[s].data_ptr()
    for k, v in (over or {}).items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    rc = lib.otvm_subjects_crop(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc, fo, to


@pytest.mark.parametrize("off", (0, 1), ids=("aligned", "offset"))
@pytest.mark.parametrize("S", COUNTS)
@pytest.mark.parametrize("H,W,h,w", SHAPES, ids=IDS)
def test_crop_equals_s_single_subject_calls(lib, H, W, h, w, S, off):
    log = _log(_origins(S, H, W, h, w))
    frame = dev(_frame_inputs(H, W, 3)[0])
    tris = [_shifted(dev(_frame_inputs(H, W, 10 + s)[1]), off) for s in range(S)]
    for fr, tr in ((frame, tris), (frame, None), (None, tris)):
        rc, fo, to = _crop_raw(lib, log[:, 1, 8:], H, W, h, w, fr, tr, off)
        assert rc == 0, lib.otvm_last_error()
        for s in range(S):
            rc1, f1, t1, _ = _crop_at_raw(lib, log[s, 1, 8:], (h, w), H, W, frame=fr, trimap=None if tr is None else tr[s])
            assert rc1 == 0
            y0, x0 = SR.clamp_origin(log[s, 1, 8:].tolist(), (h, w), H, W)            # ... and the definition, for every subject
            if fr is not None:
                assert torch.equal(fo[s], f1) and torch.equal(fo[s], frame[y0:y0 + h, x0:x0 + w]), (s, off)
            if tr is not None:
                assert np.array_equal(bits(to[s]), bits(t1)) and torch.equal(to[s], tris[s][:, y0:y0 + h, x0:x0 + w]), (s, off)
    # ... and the definition: the window at the clamped origin
    y0, x0 = SR.clamp_origin(log[S - 1, 1, 8:].tolist(), (h, w), H, W)
    assert torch.equal(to[S - 1], tris[S - 1][:, y0:y0 + h, x0:x0 + w])


def test_crop_python_wrapper(lib):
    from otvm_amd import subjects
    H, W, h, w = 37, 53, 16, 20
    log = _log(_origins(3, H, W, h, w))
    frame, tris = dev(_frame_inputs(H, W, 3)[0]), [dev(_frame_inputs(H, W, 10 + s)[1]) for s in range(3)]
    fo, to = subjects.crop(log[:, 1, 8:], (h, w), frame=frame, trimaps=tris)
    for s in range(3):
        y0, x0 = SR.clamp_origin(log[s, 1, 8:].tolist(), (h, w), H, W)
        assert torch.equal(fo[s], frame[y0:y0 + h, x0:x0 + w]) and torch.equal(to[s], tris[s][:, y0:y0 + h, x0:x0 + w])
    assert subjects.crop(log[:, 1, 8:], (h, w), frame=frame)[1] is None
    with pytest.raises(ValueError, match="one trimap per subject"):
        subjects.crop(log[:, 1, 8:], (h, w), frame=frame, trimaps=tris[:2])
    with pytest.raises(ValueError, match="1 <= h <= 37"):
        subjects.crop(log[:, 1, 8:], (38, w), frame=frame)


# ------------------------------------------------------------------------------------------------ bbox
def _class_trimaps(S, h, w, seed):
    """S one-hot trimaps [3,h,w]: random classes in a random box, the first all background (an empty box)."""
    g = np.random.default_rng(seed)
    out = []
    for s in range(S):
        cls = np.zeros((h, w), np.int64)
        if s > 0:
            y0, x0 = int(g.integers(0, h)), int(g.integers(0, w))
            y1, x1 = int(g.integers(y0, h)), int(g.integers(x0, w))
            cls[y0:y1 + 1, x0:x1 + 1] = g.choice(3, size=(y1 - y0 + 1, x1 - x0 + 1))
            if s == 2:
                cls[0, 0], cls[h - 1, w - 1] = 2, 1                        # reaches every side
        out.append(np.stack([(cls == k) for k in range(3)]).astype(np.float32))
    return out


def _bbox_raw(lib, tris, out, h, w, over=None):
    from otvm_amd import lib as L
    p = L.SubjectsBboxParams()
    p.S, p.H, p.W = len(tris), h, w
    for s, t in enumerate(tris):
        p.trimap[s] = t.data_ptr()
    p.out_base, p.out_stride = out.data_ptr(), out.stride(0)
    for k, v in (over or {}).items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    rc = lib.otvm_subjects_bbox(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("off", (0, 1), ids=("aligned", "offset"))
@pytest.mark.parametrize("S", COUNTS)
@pytest.mark.parametrize("h,w", [(16, 20), (32, 32), (37, 53), (64, 96)], ids=lambda v: str(v))
def test_bbox_equals_s_single_subject_calls(lib, h, w, S, off):
    from otvm_amd import roi
    tris_np = _class_trimaps(S, h, w, 7 * h + S)
    tris = [_shifted(dev(t), off) for t in tris_np]
    logs = [_log([(1, 2)] * S, fill) for fill in (JUNK, -JUNK)]            # two calls: equal bits whatever was there
    for log in logs:
        assert _bbox_raw(lib, tris, log[:, 1, :8], h, w) == 0, lib.otvm_last_error()
    assert torch.equal(logs[0][:, 1], logs[1][:, 1])
    assert (logs[0][:, 0] == JUNK).all() and (logs[0][:, 1, 8:] == dev(np.array([1, 2], np.int32))).all()
    for s in range(S):
        want = roi.trimap_bbox(tris[s])
        assert torch.equal(logs[0][s, 1, :8], want), (s, logs[0][s, 1, :8].tolist(), want.tolist())
        assert tuple(want.tolist()) == tuple(int(v) for v in R.bbox(tris_np[s]))
    assert tuple(logs[0][0, 1, :8].tolist()) == (h, w, -1, -1, h, w, -1, -1)


# ------------------------------------------------------------------------------------------------ resolve
def _resolve_raw(lib, origins, H, W, h, w, alphas, tris, fgrs=None, frame=None, rgb=0, normalise=0, want=ALL, off=0, over=None):
    """One otvm_subjects_resolve call on outputs pre-filled with junk -> (rc, {name: tensor})"""
    from otvm_amd import lib as L
    S = origins.shape[0]
    p = L.SubjectsResolveParams()
    p.S, p.H, p.W, p.h, p.w, p.u8_rgb, p.normalise = S, H, W, h, w, rgb, normalise
    p.origin_base, p.origin_stride = origins.data_ptr(), origins.stride(0)
    for s in range(S):
        p.win_alpha[s], p.win_trimap[s] = alphas[s].data_ptr(), tris[s].data_ptr()
        if fgrs is not None:
            p.win_fgr[s] = fgrs[s].data_ptr()
    p.frame = None if frame is None else frame.data_ptr()
    outs = {}
    for name, field, shape, dt, fill in (("alpha", "alpha", (S, H, W), torch.float32, -7.0), ("alpha_u8", "alpha_u8", (S, H, W), torch.uint8, 77),
                                         ("trimap", "trimap", (S, 3, H, W), torch.float32, -7.0),
                                         ("fgr", "fgr", (S, 3, H, W), torch.float32, -7.0), ("union", "union_alpha", (H, W), torch.float32, -7.0),
                                         ("union_u8", "union_u8", (H, W), torch.uint8, 77), ("owner", "owner", (H, W), torch.uint8, 77)):
        if name in want:
            outs[name] = _offset(shape, dt, fill, off)
            setattr(p, field, outs[name].data_ptr())
    for k, v in (over or {}).items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    rc = lib.otvm_subjects_resolve(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc, outs


def _results(S, h, w, seed):
    res = [_window_results(h, w, seed + s) for s in range(S)]             # (a NaN in the middle and an Inf at (0, 0) of each)
    return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]


@pytest.mark.parametrize("S", COUNTS)
@pytest.mark.parametrize("H,W,h,w", SHAPES, ids=IDS)
def test_resolve_without_normalise_equals_s_pastes(lib, H, W, h, w, S):
    log = _log(_origins(S, H, W, h, w))
    frame = dev(_frame_inputs(H, W, 3)[0])
    alphas, tris, fgrs = ([dev(x) for x in xs] for xs in _results(S, h, w, 40 * S))
    for with_fgr, rgb, off in ((True, 0, 0), (True, 1, 0), (False, 0, 0), (True, 0, 1), (False, 1, 1)):
        want = PLANES if with_fgr else PLANES[:3]
        rc, outs = _resolve_raw(lib, log[:, 1, 8:], H, W, h, w, alphas, tris, fgrs if with_fgr else None, frame if with_fgr else None,
                                rgb, 0, want + ("union", "union_u8", "owner"), off)
        assert rc == 0, lib.otvm_last_error()
        for s in range(S):
            rc1, one = _paste_at_raw(lib, log[s, 1, 8:], (h, w), H, W, alphas[s], tris[s], fgrs[s] if with_fgr else None,
                                     frame if with_fgr else None, rgb, None, want)
            assert rc1 == 0
            for name in want:
                assert np.array_equal(bits(outs[name][s]), bits(one[name])), (name, s, with_fgr, rgb, off)
    # every output on its own: the others are not needed for it
    rc2, both = _resolve_raw(lib, log[:, 1, 8:], H, W, h, w, alphas, tris, fgrs, frame, 0, 0, ALL)
    for name in ALL:
        rc, outs = _resolve_raw(lib, log[:, 1, 8:], H, W, h, w, alphas, tris, fgrs, frame, 0, 0, (name,))
        assert rc == 0 and rc2 == 0 and np.array_equal(bits(outs[name]), bits(both[name])), name


def _placements(H, W, h, w):
    """name -> (origins, size): windows that are disjoint, partly overlapping, identical, and equal to the frame"""
    return {"disjoint": ([(0, 0), (H - h, W - w)], (h, w)),
            "overlapping": ([(0, 0), (h // 2, w // 2), (h // 2 + 3, w // 4)], (h, w)),
            "identical": ([(4, 8)] * 3, (h, w)),
            "frame": ([(0, 0), (0, 0)], (H, W))}


def _overlap_values(S, h, w, seed):
    """Alphas whose sums over the subjects lie above 1, at exactly 1 and at 0, with a NaN and an Inf in window 0; no denormals."""
    g = np.random.default_rng(seed)
    alphas = [(g.integers(1, 256, size=(h, w)) / 256.0).astype(np.float32) for _ in range(S)]       # [1/256, 1): sums of 2+ pass 1
    for s in range(S):
        alphas[s][1, :] = 0.0                                              # a row of zeros in every window
        alphas[s][2, :] = np.float32(1.0 / S) if S in (1, 2, 4) else np.float32(0.25)               # exact sums where they coincide
        alphas[s][3, :] = 1.0
    alphas[0][0, 1], alphas[0][0, 2] = np.nan, np.inf
    alphas[S - 1][4, 0:4] = (0.75, 0.5, 0.25, 0.0)
    tris = [g.random((3, h, w)).astype(np.float32) for _ in range(S)]
    fgrs = [(g.random((3, h, w)) * 1.1).astype(np.float32) for _ in range(S)]
    return alphas, tris, fgrs


@pytest.mark.parametrize("normalise", (0, 1))
@pytest.mark.parametrize("H,W,h,w", SHAPES, ids=IDS)
def test_resolve_equals_the_restatement(lib, H, W, h, w, normalise):
    frame_np = _frame_inputs(H, W, 5)[0]
    frame = dev(frame_np)
    for name, (origins, size) in _placements(H, W, h, w).items():
        S = len(origins)
        a_np, t_np, f_np = _overlap_values(S, size[0], size[1], 17 + len(name))
        log = _log(origins)
        alphas, tris, fgrs = ([dev(x) for x in xs] for xs in (a_np, t_np, f_np))
        # (the last two: R, G, B bytes through the 16-byte form, and no F at all -- the paste shares these bodies, so "equals S
        # pastes" above does not hold them against anything)
        for rgb, off, with_fgr in ((0, 0, True), (1, 1, True), (1, 0, True), (0, 0, False)):
            want = ALL if with_fgr else tuple(k for k in ALL if k != "fgr")
            args = (fgrs, frame) if with_fgr else (None, None)
            ref = SR.resolve(origins, size, H, W, a_np, t_np, f_np if with_fgr else None, frame_np, bool(rgb), bool(normalise))
            rc, got = _resolve_raw(lib, log[:, 1, 8:], H, W, size[0], size[1], alphas, tris, *args, rgb, normalise, want, off)
            rc2, again = _resolve_raw(lib, log[:, 1, 8:], H, W, size[0], size[1], alphas, tris, *args, rgb, normalise, want, off)
            assert rc == 0 and rc2 == 0, lib.otvm_last_error()
            for k in want:
                assert np.array_equal(bits(got[k]), bits(ref[k])), (name, k, rgb, off, with_fgr)
                assert np.array_equal(bits(got[k]), bits(again[k])), (name, k)
        # what the cases are there for
        total = sum(ref["alpha"][s] for s in range(S))
        if name != "disjoint":
            over = SR.resolve(origins, size, H, W, a_np, t_np, f_np, frame_np, False, False)["alpha"].sum(0) > 1.0
            assert over.any()
            if normalise:
                assert np.nanmax(np.where(over, total, 0.0)) <= 1.0 + 1e-6 * S
        y0, x0 = origins[0]
        assert np.isnan(ref["alpha"][0, y0, x0 + 1]) and ref["alpha_u8"][0, y0, x0 + 1] == 0       # no rescaling through the NaN
        assert ref["alpha_u8"][0, y0, x0 + 2] == 0                                                  # the Inf's byte
        if name != "frame":
            assert (ref["owner"] == 255).any() and (ref["union"] == 0).any()


def test_resolve_python_wrapper(lib):
    from otvm_amd import subjects
    H, W, h, w = 37, 53, 16, 20
    origins = [(0, 0), (8, 10), (-3, 99)]
    log = _log(origins)
    a_np, t_np, f_np = _overlap_values(3, h, w, 3)
    frame_np = _frame_inputs(H, W, 5)[0]
    for normalise in (False, True):
        ref = SR.resolve(origins, (h, w), H, W, a_np, t_np, f_np, frame_np, True, normalise)
        got = subjects.resolve(log[:, 1, 8:], (h, w), H, W, [dev(x) for x in a_np], [dev(x) for x in t_np], [dev(x) for x in f_np],
                               dev(frame_np), True, normalise, ALL)
        assert sorted(got) == sorted(ALL)
        for k in ALL:
            assert np.array_equal(bits(got[k]), bits(ref[k])), (k, normalise)
    got = subjects.resolve(log[:, 1, 8:], (h, w), H, W, [dev(x) for x in a_np], [dev(x) for x in t_np])
    assert "fgr" not in got and np.array_equal(bits(got["union"]), bits(SR.resolve(origins, (h, w), H, W, a_np, t_np)["union"]))
    with pytest.raises(ValueError, match="needs every subject's fp32 F"):
        subjects.resolve(log[:, 1, 8:], (h, w), H, W, [dev(x) for x in a_np], [dev(x) for x in t_np], want=("fgr",))
    with pytest.raises(ValueError, match="at least one"):
        subjects.resolve(log[:, 1, 8:], (h, w), H, W, [dev(x) for x in a_np], [dev(x) for x in t_np], want=())


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_return_nonzero_name_the_function_and_leave_the_outputs_untouched(lib):
    H, W, h, w, S = 37, 53, 16, 20, 3
    log = _log(_origins(S, H, W, h, w))
    frame = dev(_frame_inputs(H, W, 3)[0])
    tris_full = [dev(_frame_inputs(H, W, 10 + s)[1]) for s in range(S)]
    alphas, tris, fgrs = ([dev(x) for x in xs] for xs in _results(S, h, w, 9))
    sizes = (dict(S=0), dict(S=9), dict(S=-1), dict(h=0), dict(w=0), dict(h=H + 1), dict(w=W + 1), dict(H=0), dict(W=16384))

    def refused(rc, name):
        assert rc != 0
        assert lib.otvm_last_error().decode().startswith(name + ":"), lib.otvm_last_error()

    # track
    for kw in sizes + (dict(box_base=None), dict(out_base=None), dict(hold=0), dict(hold=16384), dict(prev_base=log.data_ptr() + 2)):
        before = log.clone()
        refused(_track_raw(lib, log[:, 0, :8], log[:, 0, 8:], log[:, 1, 8:], H, W, h, w, 2, over=kw), "otvm_subjects_track")
        assert torch.equal(log, before), kw
    # crop
    for kw in sizes + (dict(origin_base=None), dict(origin_base=log.data_ptr() + 1), dict(frame=None), dict(frame_out=(1, None)),
                       dict(trimap=(2, None)), dict(trimap_out=(0, None))):
        rc, fo, to = _crop_raw(lib, log[:, 1, 8:], H, W, h, w, frame, tris_full, over=kw)
        refused(rc, "otvm_subjects_crop")
        assert all((x == 77).all() for x in fo) and all((x == -7.0).all() for x in to), kw
    rc, fo, to = _crop_raw(lib, log[:, 1, 8:], H, W, h, w, None, None)
    refused(rc, "otvm_subjects_crop")                                      # no destination
    # bbox
    for kw in (dict(S=0), dict(S=9), dict(H=0), dict(W=16384), dict(out_base=None), dict(out_base=log.data_ptr() + 2), dict(trimap=(1, None))):
        before = log.clone()
        refused(_bbox_raw(lib, tris, log[:, 1, :8], h, w, over=kw), "otvm_subjects_bbox")
        assert torch.equal(log, before), kw
    # resolve
    bad = sizes + (dict(origin_base=None), dict(origin_base=log.data_ptr() + 2), dict(win_alpha=(2, None)), dict(win_trimap=(0, None)),
                   dict(win_fgr=(1, None)), dict(frame=None), dict(win_alpha=(0, alphas[0].data_ptr() + 2)))
    for kw in bad:
        rc, outs = _resolve_raw(lib, log[:, 1, 8:], H, W, h, w, alphas, tris, fgrs, frame, 0, 1, ALL, over=kw)
        refused(rc, "otvm_subjects_resolve")
        for name, x in outs.items():
            assert (x == (-7.0 if x.dtype == torch.float32 else 77)).all(), (kw, name)
    rc, outs = _resolve_raw(lib, log[:, 1, 8:], H, W, h, w, alphas, tris, fgrs, frame, 0, 1, ())
    refused(rc, "otvm_subjects_resolve")                                   # no output requested
    rc, outs = _resolve_raw(lib, log[:, 1, 8:], H, W, h, w, alphas, tris, None, None, 0, 1, ("alpha", "fgr"))
    refused(rc, "otvm_subjects_resolve")                                   # fgr without F and without the frame
    assert (outs["alpha"] == -7.0).all() and (outs["fgr"] == -7.0).all()
    for f in (lib.otvm_subjects_track, lib.otvm_subjects_crop, lib.otvm_subjects_bbox, lib.otvm_subjects_resolve):
        assert f(None, stream()) != 0


# ------------------------------------------------------------------------------------------------ the route
H_, W_, T_, BAND, MARGIN = 96, 128, 5, 4, 8
KW = dict(skip=2, max_num=3)
SIZE = ("track", 64, 64)
CENTRES = ((30, 30), (40, 60), (62, 100))                                  # the 64x64 windows of the first two overlap; so do 2 and 3


def _subjects_clip():
    """Five frames of the synthetic clip and three disc subjects: the first-frame trimap of a soft disc of radius 12 each."""
    from otvm_amd.synth_data import synthetic_clip
    frames, _ = synthetic_clip(H_, W_, T_, seed=31)
    yy, xx = np.mgrid[0:H_, 0:W_]
    ms = [np.floor(np.clip((12 - np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)) / 3.0 + 0.5, 0, 1) * 255.0 + 0.5).astype(np.uint8) for cy, cx in CENTRES]
    return [np.ascontiguousarray(f) for f in frames], ms, [MR.trimap_from_mask(m, BAND) for m in ms]


@pytest.fixture(scope="module")
def route(lib, synth_sd, tmp_path_factory):
    """One model for all route tests, with the kernel configurations fixed and shared through a file (eval_cli's own model
    launches the same ones), and the single-subject runs every test compares with, made once."""
    from otvm_amd import engine
    from otvm_amd.video import run_video_matte
    from tests.test_gpu_frame import _fresh_model
    old, old_auto = os.environ.get("OTVM_TUNE_FILE"), engine.AUTOTUNE
    os.environ["OTVM_TUNE_FILE"] = os.path.join(str(tmp_path_factory.mktemp("tune")), "tune.json")
    engine.AUTOTUNE = False
    try:
        m = _fresh_model(synth_sd, 12, "f16x3")
        frames, ms, tris = _subjects_clip()
        singles = [run_video_matte(m, frames, trimap=t, roi=SIZE, roi_margin=MARGIN, **KW) for t in tris]
        yield m, frames, ms, tris, singles
    finally:
        engine.AUTOTUNE = old_auto
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a.contiguous()), bits(b.contiguous()))


def _ref_over_singles(singles, normalise):
    """union, owner and the per-subject alphas of the restatement applied, frame by frame, to the single runs' full-frame planes
    (the window is the frame: every plane is already pasted)."""
    out = []
    for t in range(T_):
        out.append(SR.resolve([(0, 0)] * len(singles), (H_, W_), H_, W_, [s["alpha"][t].numpy() for s in singles],
                              [s["trimap"][t].numpy() for s in singles], normalise=normalise))
    return out


def test_route_equals_the_single_subject_runs(route):
    from otvm_amd.subjects import run_video_matte_subjects
    m, frames, ms, tris, singles = route
    got = run_video_matte_subjects(m, frames, tris, roi=SIZE, roi_margin=MARGIN, **KW)
    assert got["alpha"].shape == (3, T_, H_, W_) and got["trimap"].shape == (3, T_, 3, H_, W_) and got["owner"].dtype == torch.uint8
    assert got["roi_size"] == (64, 64) and len(got["bank_frames"]) == T_
    for s, one in enumerate(singles):
        assert _eq(got["alpha"][s], one["alpha"]), s
        assert _eq(got["alpha_u8"][s], one["alpha_u8"]) and _eq(got["trimap"][s], one["trimap"]), s
        assert got["roi"][s] == one["roi"] and got["roi_clipped"][s] == one["roi_clipped"], s
    wins = [got["roi"][s][0] for s in range(3)]
    overlap = lambda a, b: abs(a[0] - b[0]) < 64 and abs(a[1] - b[1]) < 64          # noqa: E731
    assert overlap(wins[0], wins[1]) and not overlap(wins[0], wins[2])
    for normalise in (False, True):
        if normalise:
            got = run_video_matte_subjects(m, frames, tris, roi=SIZE, roi_margin=MARGIN, overlap="normalise", **KW)
        ref = _ref_over_singles(singles, normalise)
        for t in range(T_):
            for k in ("union", "union_u8", "owner"):
                assert np.array_equal(bits(got[k][t]), bits(ref[t][k])), (k, t, normalise)
            for k in ("alpha", "alpha_u8"):
                assert np.array_equal(bits(got[k][:, t]), bits(ref[t][k])), (k, t, normalise)
            assert _eq(got["trimap"][:, t], torch.stack([one["trimap"][t] for one in singles]))     # never rescaled


def test_route_picks_the_size_the_host_rule_gives(route):
    from otvm_amd import roi
    from otvm_amd.subjects import run_video_matte_subjects
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, singles = route
    boxes = [tuple(int(v) for v in R.bbox(t)[4:]) for t in tris]
    size = roi.window_size(boxes, H_, W_, MARGIN)
    assert size == R.window_size(boxes, H_, W_, MARGIN) and size != (H_, W_)
    got = run_video_matte_subjects(m, frames[:2], tris[:2], roi="track", roi_margin=MARGIN, **KW)
    assert got["roi_size"] == size
    for s in range(2):
        assert got["roi"][s][0] == roi.window_origin(boxes[s], size[0], size[1], H_, W_) + size
    assert size == (64, 64)                                                # (33-pixel boxes, 8 pixels round them, rounded up to 32)
    for s in range(2):
        one = run_video_matte(m, frames[:2], trimap=tris[s], roi=SIZE, roi_margin=MARGIN, **KW)
        assert _eq(got["alpha"][s], one["alpha"]) and got["roi"][s] == one["roi"]
    with pytest.raises(ValueError, match="does not hold the trimap of subject 0"):
        run_video_matte_subjects(m, frames, tris, roi=("track", 16, 64), **KW)


def test_route_without_windows_equals_the_plain_runs(route):
    from otvm_amd.subjects import run_video_matte_subjects
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, singles = route
    got = run_video_matte_subjects(m, frames[:3], tris[:2], roi=None, **KW)
    assert got["roi_size"] == (H_, W_) and got["roi"] == [[(0, 0, H_, W_)] * 3] * 2 and got["roi_clipped"] == [[], []]
    for s in range(2):
        one = run_video_matte(m, frames[:3], trimap=tris[s], **KW)
        assert _eq(got["alpha"][s], one["alpha"]) and _eq(got["alpha_u8"][s], one["alpha_u8"]) and _eq(got["trimap"][s], one["trimap"]), s


def test_route_foreground_equals_the_single_subject_runs(route):
    from otvm_amd.subjects import run_video_matte_subjects
    from otvm_amd.video import run_video_matte
    m, frames, ms, tris, singles = route
    got = run_video_matte_subjects(m, frames[:3], tris, roi=SIZE, roi_margin=MARGIN, foreground=True, **KW)
    assert got["fgr_u8"].shape == (3, 3, H_, W_, 4) and m.module.foreground is False
    for s in range(3):
        one = run_video_matte(m, frames[:3], trimap=tris[s], roi=SIZE, roi_margin=MARGIN, foreground=True, **KW)
        assert _eq(got["fgr_u8"][s], one["fgr_u8"]) and _eq(got["alpha"][s], one["alpha"]), s
        assert torch.equal(got["fgr_u8"][s][..., 3], got["alpha_u8"][s])


def test_the_frame_loop_reads_nothing_back_and_its_launches_do_not_grow_with_s(route, monkeypatch):
    from otvm_amd import roi, subjects
    m, frames, ms, tris, singles = route
    events, real = [], subjects.rows_of

    def counted(buf):
        events.append("read")
        return real(buf)

    def never(*a):
        raise AssertionError("the route reads back through subjects.rows_of alone")
    monkeypatch.setattr(subjects, "rows_of", counted)
    monkeypatch.setattr(roi, "rows_of", never)
    monkeypatch.setattr(roi, "boxes_of", never)
    calls = {}
    for name in ("track", "crop", "bbox", "resolve"):
        def wrapped(*a, _f=getattr(subjects, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(subjects, name, wrapped)
    counts = {}
    for S in (1, 3):
        events.clear(), calls.clear()
        got = subjects.run_video_matte_subjects(m, frames, tris[:S], roi=SIZE, roi_margin=MARGIN, keep_on_device=True,
                                                on_frame=lambda t, a, u, o: events.append(t), **KW)
        assert events == ["read"] + list(range(T_)) + ["read"], S
        assert got["alpha"].is_cuda and got["alpha"].shape[0] == S
        counts[S] = dict(calls)
    # (bbox: once more before the first frame, for the subjects' own boxes)
    assert counts[1] == counts[3] == dict(track=T_, crop=T_, bbox=T_ + 1, resolve=T_)


# ------------------------------------------------------------------------------------------------ eval_cli
def test_eval_cli_subjects(tmp_path, route):
    from PIL import Image
    from otvm_amd import eval_cli
    from otvm_amd.subjects import run_video_matte_subjects
    m, frames_bgr, ms, tris, singles = route
    demo = os.path.join(str(tmp_path), "demo")
    names = ("ann", "bob", "cy")
    os.makedirs(os.path.join(demo, "clip", "frames"))
    for t in range(T_):
        Image.fromarray(frames_bgr[t][..., ::-1].copy()).save(os.path.join(demo, "clip", "frames", "%04d.png" % t))
    for n, tri in zip(names, tris):
        os.makedirs(os.path.join(demo, "clip", "subjects", n))
        grey = (tri[1] * 128 + tri[2] * 255).astype(np.uint8)
        Image.fromarray(grey).save(os.path.join(demo, "clip", "subjects", n, "0000.png"))
    common = ["--demo", "--data", demo, "--synthetic-weights", "--skip", "2", "--max-num", "3"]
    out = os.path.join(str(tmp_path), "out")
    res = eval_cli.main(common + ["--out", out, "--subjects", "--roi", "track,64,64", "--roi-margin", str(MARGIN), "--fgr",
                                  "--subjects-overlap", "normalise"])
    assert res["frames"] == T_
    ref = run_video_matte_subjects(m, frames_bgr, tris, roi=SIZE, roi_margin=MARGIN, overlap="normalise", foreground=True, **KW)
    pred = os.path.join(out, "alpha", "test", "s4_OTVM", "pred", "clip")
    for t in range(T_):
        assert np.array_equal(np.asarray(Image.open(os.path.join(pred, "%04d.png" % t))), ref["union_u8"][t].numpy()), t
        for s, n in enumerate(names):
            assert np.array_equal(np.asarray(Image.open(os.path.join(pred, n, "%04d.png" % t))), ref["alpha_u8"][s, t].numpy()), (n, t)
            rgba = np.asarray(Image.open(os.path.join(out, "fgr", "clip", n, "%04d.png" % t)))
            assert rgba.shape == (H_, W_, 4) and np.array_equal(rgba[..., 3], ref["alpha_u8"][s, t].numpy())
            assert np.array_equal(rgba[..., :3], ref["fgr_u8"][s, t].numpy()[..., 2::-1]), (n, t)
    for argv, word in ((["--subjects", "--roi", "auto"], "--roi"), (["--subjects", "--roi", "0,0,64,64"], "--roi"),
                       (["--subjects", "--keyframes"], "--keyframes"), (["--subjects", "--batch", "2"], "--batch")):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(common + ["--out", out] + argv)
        assert word in str(e.value), (argv, str(e.value))
