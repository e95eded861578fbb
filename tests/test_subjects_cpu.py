"""Multi-subject matting without a GPU: the binding of the four entry points (the header's prototypes and structs, refusals before
any launch, ABI still 21), the host-side refusals of run_video_matte_subjects and of eval_cli --subjects, the one window size of
several boxes, and the properties of the resolve's restatement (tests/subjects_ref.py)."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import subjects_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("otvm_subjects_track", "otvm_subjects_crop", "otvm_subjects_bbox", "otvm_subjects_resolve")


# ------------------------------------------------------------------ the binding
def _header_fields(header, struct):
    body = header[header.index("typedef struct %s {" % struct):header.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl.strip())
        names += [re.sub(r"\[.*\]", "", x).strip().lstrip("*") for x in decl.split(",") if x.strip()]
    return names


def test_header_declares_and_lib_binds_the_four_entry_points():
    import __graft_entry__ as g
    from otvm_amd import lib as L
    h = ctypes.CDLL(g.build())
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    for sym in ENTRY:
        assert sym in L.EXPORTED and getattr(h, sym) is not None
        assert re.search(r"\bint %s\(const %s_params\* p, void\* stream\);" % (sym, sym), header), sym
    h.otvm_abi_version.restype = ctypes.c_int
    assert h.otvm_abi_version() == 21 == L.ABI_VERSION and "#define OTVM_ABI_VERSION 21 " in header
    assert "#define OTVM_SUBJECTS_MAX 8\n" in header and L.SUBJECTS_MAX == 8
    for struct, T in (("otvm_subjects_track_params", L.SubjectsTrackParams), ("otvm_subjects_crop_params", L.SubjectsCropParams),
                      ("otvm_subjects_bbox_params", L.SubjectsBboxParams), ("otvm_subjects_resolve_params", L.SubjectsResolveParams)):
        assert _header_fields(header, struct) == [f for f, _ in T._fields_], struct
    # the tracking window's structs are taken as they are
    assert (ctypes.sizeof(L.RoiBboxParams), ctypes.sizeof(L.RoiCropParams), ctypes.sizeof(L.RoiPasteParams), ctypes.sizeof(L.RoiTrackParams)) == (32, 72, 104, 48)


def test_the_new_structs_have_the_sizes_gcc_gives_them():
    from otvm_amd import lib as L
    structs = (("otvm_subjects_track_params", L.SubjectsTrackParams, "hold"), ("otvm_subjects_crop_params", L.SubjectsCropParams, "trimap_out"),
               ("otvm_subjects_bbox_params", L.SubjectsBboxParams, "out_stride"), ("otvm_subjects_resolve_params", L.SubjectsResolveParams, "owner"))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "otvm_hip.h"\nint main(void) {\n'
    for name, _, last in structs:
        src += 'printf("%%zu %%zu ", sizeof(%s), offsetof(%s, %s));\n' % (name, name, last)
    src += "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, T, last in structs:
        want += [ctypes.sizeof(T), getattr(T, last).offset]
    assert got == want


def test_bad_arguments_are_refused_before_any_launch():
    """The checks precede the launch, so they answer without a device: nonzero, and the message starts with the function's name."""
    import __graft_entry__ as g
    from otvm_amd import lib as L
    g.build()
    lib = L.load()
    buf = (ctypes.c_float * 256)()
    at = ctypes.addressof(buf)

    def refused(rc, name):
        assert rc != 0
        assert lib.otvm_last_error().decode().startswith(name + ":"), lib.otvm_last_error()

    def apply(p, kw):
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
    sizes = (dict(S=0), dict(S=9), dict(h=0), dict(w=0), dict(h=9), dict(w=13), dict(H=0), dict(W=0), dict(H=16384), dict(W=16384), dict(h=-1))
    for kw in sizes + (dict(box_base=None), dict(out_base=None), dict(hold=0), dict(hold=16384), dict(prev_base=at + 2), dict(box_base=at + 1)):
        p = L.SubjectsTrackParams()
        p.S, p.box_base, p.box_stride, p.prev_base, p.prev_stride, p.out_base, p.out_stride = 2, at, 10, at + 32, 10, at + 128, 10
        p.H, p.W, p.h, p.w, p.hold = 8, 12, 4, 4, 2
        apply(p, kw)
        refused(lib.otvm_subjects_track(ctypes.byref(p), None), "otvm_subjects_track")
    for kw in sizes + (dict(origin_base=None), dict(origin_base=at + 2), dict(frame=None), dict(frame_out=(1, None)), dict(trimap_out=(0, at)),
                       dict(trimap_out=(0, at), trimap=(0, at))):
        p = L.SubjectsCropParams()
        p.S, p.H, p.W, p.h, p.w, p.origin_base, p.origin_stride, p.frame = 2, 8, 12, 4, 4, at, 2, at
        p.frame_out[0], p.frame_out[1] = at, at
        apply(p, kw)
        refused(lib.otvm_subjects_crop(ctypes.byref(p), None), "otvm_subjects_crop")
    for kw in (dict(S=0), dict(S=9), dict(H=0), dict(W=16384), dict(out_base=None), dict(out_base=at + 2), dict(trimap=(1, None)), dict(trimap=(0, at + 1))):
        p = L.SubjectsBboxParams()
        p.S, p.H, p.W, p.out_base, p.out_stride = 2, 8, 12, at, 10
        p.trimap[0], p.trimap[1] = at, at
        apply(p, kw)
        refused(lib.otvm_subjects_bbox(ctypes.byref(p), None), "otvm_subjects_bbox")
    for kw in sizes + (dict(alpha=None), dict(origin_base=None), dict(origin_base=at + 1), dict(win_alpha=(1, None)), dict(win_trimap=(0, None)),
                       dict(fgr=at), dict(fgr=at, frame=at), dict(fgr=at, frame=at, win_fgr=(0, at)), dict(fgr=at, win_fgr=(0, at)),
                       dict(union_alpha=at + 2), dict(win_alpha=(0, at + 3))):
        p = L.SubjectsResolveParams()
        p.S, p.H, p.W, p.h, p.w, p.origin_base, p.origin_stride, p.alpha = 2, 8, 12, 4, 4, at, 2, at
        for s in range(2):
            p.win_alpha[s], p.win_trimap[s] = at, at
        apply(p, kw)
        refused(lib.otvm_subjects_resolve(ctypes.byref(p), None), "otvm_subjects_resolve")
    for name in ENTRY:
        refused(getattr(lib, name)(None, None), name)


# ------------------------------------------------------------------ refusals that need no device
class _NoDevice(torch.nn.Module):
    DILATION_KERNEL = 12

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0
        self.precision = None

    def forward(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the model was touched")

    forward_batch = forward


def test_route_refusals_come_before_the_model_or_the_device_is_touched(monkeypatch):
    from otvm_amd.masks import Mask
    from otvm_amd.subjects import run_video_matte_subjects

    def no_cuda(*a, **kw):
        raise AssertionError("a CUDA call was made")
    monkeypatch.setattr(torch.cuda, "current_stream", no_cuda)
    monkeypatch.setattr(torch.Tensor, "cuda", no_cuda)
    model = _NoDevice()
    H, W, T = 40, 48, 3
    frames = [np.zeros((H, W, 3), np.uint8)] * T
    tri = np.zeros((3, H, W), np.float32)
    for kw, word in ((dict(frames=[f.astype(np.float32) for f in frames]), "float frames"),
                     (dict(subjects=[]), "1 .. 8"), (dict(subjects=[tri] * 9), "1 .. 8"), (dict(subjects=tri), "1 .. 8"),
                     (dict(subjects=[tri, np.zeros((3, H, W + 1), np.float32)]), "resolution"),
                     (dict(subjects=[np.zeros((3, H + 2, W), np.float32)]), "subjects are 42x48"),
                     (dict(subjects=[np.zeros((H, W), np.float32)]), "one-hot trimap"),
                     (dict(subjects=[Mask(np.zeros((H, W), np.uint8), role="labels")]), "role"),
                     (dict(roi="auto"), "'auto'"), (dict(roi=(0, 0, 32, 32)), "static window"), (dict(roi="follow"), "'track'"),
                     (dict(roi=("track", 0, 32)), "h, w >= 1"), (dict(roi=("track", 32.5, 32)), "h, w >= 1"),
                     (dict(roi_margin=-1), "roi_margin"), (dict(roi_margin=True), "roi_margin"), (dict(overlap="max"), "overlap"),
                     (dict(frames=[]), "no frames")):
        args = dict(frames=frames, subjects=[tri, tri])
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            run_video_matte_subjects(model, args.pop("frames"), args.pop("subjects"), **args)
    for precision in ("f32", "f16", "bf16"):
        model.precision = precision
        with pytest.raises(ValueError, match="f16x3"):
            run_video_matte_subjects(model, frames, [tri])
    model.precision = None
    assert model.calls == 0


def test_eval_cli_subjects_refusals(tmp_path):
    from otvm_amd import eval_cli
    data = str(tmp_path)
    for argv, word in ((["--subjects"], "--demo"), (["--demo", "--subjects-overlap", "keep"], "--subjects"),
                       (["--demo", "--subjects", "--roi", "auto"], "--roi"), (["--demo", "--subjects", "--roi", "0,0,32,32"], "--roi"),
                       (["--demo", "--subjects", "--keyframes"], "--keyframes"), (["--demo", "--subjects", "--masks", "key"], "--masks"),
                       (["--demo", "--subjects", "--work-scale", "2"], "--work-scale"), (["--demo", "--subjects", "--stabilise"], "--stabilise"),
                       (["--demo", "--subjects", "--viz"], "--viz"), (["--demo", "--subjects", "--composite", "1,2,3"], "--composite"),
                       (["--demo", "--subjects", "--batch", "2"], "--batch"), (["--demo", "--subjects", "--roi", "track,0,5"], "--roi")):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(["--data", data, "--synthetic-weights"] + argv)
        assert word in str(e.value) and "eval_cli" in str(e.value), (argv, str(e.value))


# ------------------------------------------------------------------ the one window size
def test_one_window_size_from_several_boxes():
    from otvm_amd import roi, subjects
    from tests import roi_ref as R
    H, W = 1080, 1920
    boxes = [(100, 200, 399, 349), (500, 900, 620, 1399), (H, W, -1, -1)]          # 300x150, 121x500 and an empty one
    assert subjects.shared_size(boxes, ("track",), 32, H, W) == (384, 576) == roi.window_size(boxes, H, W, 32) == R.window_size(boxes, H, W, 32)
    assert subjects.shared_size(boxes, ("track",), 0, H, W) == (320, 512)          # the largest extent per axis, not the union's
    assert subjects.shared_size([(0, 0, 1079, 10)], ("track",), 32, H, W) == (1080, 96)          # never larger than the frame
    assert subjects.shared_size([(H, W, -1, -1)], ("track",), 32, H, W) == (32, 32)
    assert subjects.shared_size(boxes, ("track", 512, 640), 32, H, W) == (512, 640)
    with pytest.raises(ValueError, match="does not hold the trimap of subject 1"):
        subjects.shared_size(boxes, ("track", 512, 499), 32, H, W)
    with pytest.raises(ValueError, match="1 <= h <= 1080"):
        subjects.shared_size(boxes, ("track", 1081, 640), 32, H, W)
    assert subjects.check_roi(None, 32) == (None, 32) and subjects.check_roi("track", 8) == (("track",), 8)
    assert subjects.check_roi(["track", 64, 96], 0) == (("track", 64, 96), 0)


# ------------------------------------------------------------------ the restatement's own properties
def _case(seed, S, H=24, W=30, h=12, w=14):
    g = np.random.default_rng(seed)
    origins = [(int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))) for _ in range(S)]
    alphas = [(g.integers(0, 257, size=(h, w)) / 256.0).astype(np.float32) for _ in range(S)]
    tris = [g.random((3, h, w)).astype(np.float32) for _ in range(S)]
    return origins, (h, w), H, W, alphas, tris


def test_restatement_normalised_alphas_sum_to_at_most_one():
    for S in (1, 2, 3, 8):
        origins, size, H, W, alphas, tris = _case(S, S)
        keep = SR.resolve(origins, size, H, W, alphas, tris, normalise=False)
        norm = SR.resolve(origins, size, H, W, alphas, tris, normalise=True)
        total = norm["alpha"].astype(np.float64).sum(0)
        assert total.max() <= 1.0 + S * 2.0 ** -24                                  # each quotient is off by half an ulp at most
        over = keep["alpha"].astype(np.float64).sum(0) > 1.0
        assert S == 1 or over.any()
        assert np.array_equal(norm["alpha"][:, ~over], keep["alpha"][:, ~over])      # nothing else is touched
        assert np.array_equal(norm["union"], keep["union"]) and np.array_equal(norm["trimap"], keep["trimap"])
        assert keep["union"].max() <= 1.0 and np.array_equal(keep["union"] == 0, keep["alpha"].max(0) == 0)


def test_restatement_without_overlap_normalise_changes_nothing():
    H, W, h, w = 24, 30, 12, 14
    _, size, _, _, alphas, tris = _case(5, 2)
    origins = [(0, 0), (12, 16)]
    keep = SR.resolve(origins, size, H, W, alphas, tris, normalise=False)
    norm = SR.resolve(origins, size, H, W, alphas, tris, normalise=True)
    for k in ("alpha", "alpha_u8", "trimap", "union", "union_u8", "owner"):
        assert np.array_equal(keep[k], norm[k]), k
    # every plane is the single-subject paste
    from tests import roi_ref as R
    for s in range(2):
        a, u8, tri, _ = R.paste(origins[s] + size, H, W, alphas[s], tris[s])
        assert np.array_equal(keep["alpha"][s], a) and np.array_equal(keep["alpha_u8"][s], u8) and np.array_equal(keep["trimap"][s], tri)


def test_restatement_owner_ties_go_to_the_smaller_index():
    H, W, h, w = 6, 8, 4, 4
    a = np.full((h, w), 0.5, np.float32)
    b = a.copy()
    b[0, 0], b[1, 1], b[2, 2] = 0.75, 0.25, 0.0
    tris = [np.zeros((3, h, w), np.float32)] * 3
    got = SR.resolve([(1, 2)] * 3, (h, w), H, W, [a, b, a.copy()], tris)
    own = got["owner"][1:5, 2:6]
    assert own[0, 0] == 1 and own[1, 1] == 0 and own[2, 2] == 0 and own[3, 3] == 0 and (got["owner"][0] == 255).all()
    zero = SR.resolve([(1, 2)] * 2, (h, w), H, W, [np.zeros((h, w), np.float32)] * 2, tris[:2])
    assert (zero["owner"] == 255).all() and (zero["union"] == 0).all()
    # a NaN owns nothing and is not rescaled through; the stale origin is clamped
    c = a.copy()
    c[0, 0] = np.nan
    got = SR.resolve([(1, 2), (-5, 99)], (h, w), H, W, [c, a], tris[:2], normalise=True)
    assert got["owner"][1, 2] == 255 and np.isnan(got["alpha"][0, 1, 2]) and got["alpha_u8"][0, 1, 2] == 0 and got["union"][1, 2] == 1.0
    assert SR.clamp_origin((-5, 99), (h, w), H, W) == (0, 4) and (got["alpha"][1, 0:4, 4:8] == 0.5).all()
