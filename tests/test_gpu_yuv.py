"""GPU (-m gpu): video streams -- otvm_yuv_to_rgb and otvm_rgb_to_yuv420 (csrc/yuv.hip) against their numpy restatement
(tests/yuv_ref.py) bit for bit, and the layers above them: yuv.Y4MFrames as the frames of run_video_matte, yuv.Y4MWriter as its
sink, python -m otvm_amd.y4m_cli end to end.  The restatement itself is held to the float64 definition in tests/test_yuv_cpu.py."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import yuv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 2), (3, 5), (7, 9), (16, 64), (33, 65), (100, 150)]
MATRICES, RANGES = ("601", "709"), ("limited", "full")
SENTINEL = 0xA5


def _lib():
    from otvm_amd import lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def sitings(layout):
    return ("left", "centre") if R.SUBSAMPLING[layout][0] else ("left",)


def _place(planes, pad, offset):
    """The planes (2-D uint8 arrays; None skipped) in ONE device buffer of junk, every plane ``offset`` bytes past a 16-byte
    boundary with rows ``pad`` bytes longer than they need be -> (buffer, [(pointer, stride)])."""
    rng_ = np.random.default_rng(99)
    chunks, where, pos = [], [], 0
    for p in planes:
        if p is None:
            where.append((0, 0))
            continue
        p = p.reshape(p.shape[0], -1)
        stride = p.shape[1] + pad
        block = rng_.integers(0, 256, offset + p.shape[0] * stride + 16, dtype=np.uint8)
        rows = block[offset:offset + p.shape[0] * stride].reshape(p.shape[0], stride)
        rows[:, :p.shape[1]] = p
        block = np.concatenate([block, np.zeros((-len(block)) % 16, np.uint8)])
        where.append((pos + offset, stride))
        chunks.append(block)
        pos += len(block)
    buf = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, [(buf.data_ptr() + o if s else 0, s) for o, s in where]


def device_to_rgb(y, u, v, layout, matrix, rng, siting, rgb, pad=0, offset=0):
    """otvm_yuv_to_rgb through the C ABI into an output pre-filled with a sentinel; nothing outside H*W*3 may change."""
    from otvm_amd import yuv
    L, lib = _lib()
    H, W = y.shape
    buf, where = _place([y, u, v], pad, offset)
    out = torch.full((offset + H * W * 3 + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    p = L.YuvToRgbParams(H=H, W=W, layout=yuv.LAYOUTS[layout], matrix=yuv.MATRICES[matrix], range=yuv.RANGES[rng],
                         siting=yuv.SITINGS[siting], y_stride=where[0][1], u_stride=where[1][1], v_stride=where[2][1], u8_rgb=int(rgb),
                         y=where[0][0], u=where[1][0] or None, v=where[2][0] or None, rgb=out.data_ptr() + offset)
    L.check(lib.otvm_yuv_to_rgb(C.byref(p), _stream()), "yuv_to_rgb")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:offset] == SENTINEL).all() and (o[offset + H * W * 3:] == SENTINEL).all()
    return o[offset:offset + H * W * 3].reshape(H, W, 3)


def device_to_yuv420(img, matrix, rng, rgb, pad=0, offset=0, gap=16):
    """otvm_rgb_to_yuv420 into one frame buffer of sentinels: [offset | Y | gap | U | gap | V | gap], rows ``pad`` longer than
    needed; everything that is no plane element must keep the sentinel.  -> (y, u, v)"""
    from otvm_amd import yuv
    L, lib = _lib()
    H, W = img.shape[:2]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    shapes, spans, pos = [(H, W), (ch, cw), (ch, cw)], [], offset
    for r, c in shapes:
        spans.append((pos, r, c, c + pad))
        pos += r * (c + pad) + gap
    out = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=DEV)
    src = torch.zeros(H * W * 3 + offset, dtype=torch.uint8, device=DEV)
    src[offset:] = torch.from_numpy(np.ascontiguousarray(img)).to(DEV).reshape(-1)
    base = out.data_ptr()
    p = L.RgbToYuv420Params(H=H, W=W, matrix=yuv.MATRICES[matrix], range=yuv.RANGES[rng], y_stride=spans[0][3], u_stride=spans[1][3],
                            v_stride=spans[2][3], u8_rgb=int(rgb), img=src.data_ptr() + offset, y=base + spans[0][0],
                            u=base + spans[1][0], v=base + spans[2][0])
    L.check(lib.otvm_rgb_to_yuv420(C.byref(p), _stream()), "rgb_to_yuv420")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    keep = np.ones(len(o), bool)
    planes = []
    for start, r, c, stride in spans:
        rows = o[start:start + r * stride].reshape(r, stride)
        planes.append(rows[:, :c].copy())
        mask = keep[start:start + r * stride].reshape(r, stride)
        mask[:, :c] = False
    assert (o[keep] == SENTINEL).all(), "bytes outside the planes were written"
    return planes


# ------------------------------------------------------------------------------------------------ otvm_yuv_to_rgb
@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_yuv_to_rgb_equals_the_restatement(layout, H, W):
    rng_ = np.random.default_rng(H * 1000 + W)
    y, u, v = R.random_planes(rng_, H, W, layout)
    for siting in sitings(layout):
        for matrix in MATRICES:
            for rng in RANGES:
                for rgb in (True, False):
                    got = device_to_rgb(y, u, v, layout, matrix, rng, siting, rgb)
                    assert np.array_equal(got, R.yuv_to_rgb(y, u, v, layout, matrix, rng, siting, rgb)), (siting, matrix, rng, rgb)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_yuv_to_rgb_padded_strides_and_odd_offsets(layout):
    for (H, W), pad, offset in (((33, 65), 3, 1), ((7, 9), 5, 3), ((16, 64), 4, 1), ((100, 150), 2, 2)):
        y, u, v = R.random_planes(np.random.default_rng(W), H, W, layout, corners=H == 7)
        for siting in sitings(layout):
            got = device_to_rgb(y, u, v, layout, "709", "limited", siting, True, pad=pad, offset=offset)
            assert np.array_equal(got, R.yuv_to_rgb(y, u, v, layout, "709", "limited", siting, True)), (H, W, siting)


@pytest.mark.parametrize("layout,siting", [("nv12", "left"), ("420p", "centre")])
def test_yuv_to_rgb_1080p_every_element(layout, siting):
    y, u, v = R.random_planes(np.random.default_rng(1080), 1080, 1920, layout)
    got = device_to_rgb(y, u, v, layout, "709", "limited", siting, True)
    assert np.array_equal(got, R.yuv_to_rgb(y, u, v, layout, "709", "limited", siting, True))


def test_yuv_to_rgb_wrapper_takes_views():
    """yuv.yuv_to_rgb on an NV12 surface that lives in a pitched allocation (rows longer than the picture)."""
    from otvm_amd import yuv
    H, W, pitch = 33, 65, 128
    y, uv, _ = R.random_planes(np.random.default_rng(2), H, W, "nv12")
    surf = torch.zeros((H + 17, pitch), dtype=torch.uint8, device=DEV)
    surf[:H, :W] = torch.from_numpy(y).to(DEV)
    surf[H:H + 17, :66] = torch.from_numpy(uv.reshape(17, 66)).to(DEV)
    got = yuv.yuv_to_rgb(surf[:H, :W], surf[H:H + 17, :66].unflatten(1, (33, 2)), layout="nv12", matrix="601", range="full", siting="left")
    assert np.array_equal(got.cpu().numpy(), R.yuv_to_rgb(y, uv, None, "nv12", "601", "full", "left"))
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(surf[:H, :W], surf[:3, :4], surf[:3, :4], layout="420p")


# ------------------------------------------------------------------------------------------------ otvm_rgb_to_yuv420
@pytest.mark.parametrize("H,W", SIZES + [(1080, 1920)], ids=["%dx%d" % s for s in SIZES + [(1080, 1920)]])
def test_rgb_to_yuv420_equals_the_restatement(H, W):
    rng_ = np.random.default_rng(H * 1000 + W + 1)
    img = rng_.integers(0, 256, (H, W, 3), dtype=np.uint8)
    cases = [("709", "limited", True)] if H == 1080 else [(m, r, o) for m in MATRICES for r in RANGES for o in (True, False)]
    for matrix, rng, rgb in cases:
        want = R.rgb_to_yuv420(img, matrix, rng, rgb)
        for pad, offset in ((0, 0),) if H == 1080 else ((0, 0), (3, 1)):
            got = device_to_yuv420(img, matrix, rng, rgb, pad=pad, offset=offset)
            for g, w, name in zip(got, want, "yuv"):
                assert np.array_equal(g, w), (name, matrix, rng, rgb, pad)


def test_rgb_to_yuv420_wrapper_writes_one_contiguous_frame():
    from otvm_amd import yuv
    H, W = 33, 65
    img = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    n = yuv.frame_bytes(H, W, "420p")
    out = torch.full((n + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    frame, (y, u, v) = yuv.rgb_to_yuv420(torch.from_numpy(img).to(DEV), matrix="601", range="full", order="bgr", out=out[:n])
    o = out.cpu().numpy()
    assert o[:n].tobytes() == R.pack_frame(*R.rgb_to_yuv420(img, "601", "full", rgb=False)) and (o[n:] == SENTINEL).all()
    assert tuple(y.shape) == (H, W) and tuple(u.shape) == tuple(v.shape) == (17, 33) and frame.data_ptr() == out.data_ptr()


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_nothing_is_launched():
    L, lib = _lib()
    H, W = 8, 8
    src = torch.zeros(H * W * 3, dtype=torch.uint8, device=DEV)
    out = torch.full((H * W * 3,), SENTINEL, dtype=torch.uint8, device=DEV)
    s, o = src.data_ptr(), out.data_ptr()

    def to_rgb(**kw):
        base = dict(H=H, W=W, layout=L.YUV_420P, matrix=0, range=0, siting=0, y_stride=W, u_stride=4, v_stride=4, u8_rgb=1, y=s, u=s, v=s, rgb=o)
        base.update(kw)
        return L.YuvToRgbParams(**base)

    def to_yuv(**kw):
        base = dict(H=H, W=W, matrix=0, range=0, y_stride=W, u_stride=4, v_stride=4, u8_rgb=1, img=s, y=o, u=o + 64, v=o + 80)
        base.update(kw)
        return L.RgbToYuv420Params(**base)

    for kw in (dict(H=0), dict(W=-3), dict(layout=9), dict(matrix=2), dict(range=-1), dict(siting=5), dict(y=None), dict(u=None), dict(v=None),
               dict(y_stride=W - 1), dict(u_stride=3), dict(v_stride=3), dict(layout=L.YUV_NV12, u_stride=7), dict(layout=L.YUV_444P, v_stride=7)):
        assert lib.otvm_yuv_to_rgb(C.byref(to_rgb(**kw)), _stream()) != 0 and lib.otvm_last_error().decode().startswith("otvm_yuv_to_rgb"), kw
    assert lib.otvm_yuv_to_rgb(C.byref(to_rgb(rgb=None)), _stream()) != 0
    for kw in (dict(H=0), dict(W=0), dict(matrix=3), dict(range=2), dict(img=None), dict(u=None), dict(y_stride=W - 1), dict(u_stride=3), dict(v_stride=0)):
        assert lib.otvm_rgb_to_yuv420(C.byref(to_yuv(**kw)), _stream()) != 0 and lib.otvm_last_error().decode().startswith("otvm_rgb_to_yuv420"), kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert lib.otvm_yuv_to_rgb(C.byref(to_rgb()), _stream()) == 0                        # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != SENTINEL).any()


# ------------------------------------------------------------------------------------------------ run_video_matte, writer, y4m_cli
H_, W_, T_ = 100, 150, 4
RUN = dict(skip=2, max_num=3, frames_are_rgb=True)


def _write_clip(path, frames_bgr):
    """The clip as a C420mpeg2 Y4M made by the restatement's forward conversion -> the RGB host arrays the restatement converts
    that file back to (BT.601 -- H < 720 -- limited range, left-sited chroma)."""
    from otvm_amd import yuv
    back = []
    with open(path, "wb") as f:
        f.write(yuv.format_y4m_header(W_, H_, "25:1", C="420mpeg2"))
        for fr in frames_bgr:
            y, u, v = R.rgb_to_yuv420(fr, "601", "limited", rgb=False)
            f.write(b"FRAME\n" + R.pack_frame(y, u, v))
            back.append(R.yuv_to_rgb(y, u, v, "420p", "601", "limited", "left", rgb=True))
    return back


@pytest.fixture(scope="module")
def route(synth_sd, tmp_path_factory):
    """One model for all route tests, in one process, with the kernel configurations fixed (no timing runs; y4m_cli's own model
    launches the same ones), the synthetic clip as a Y4M file and as the host arrays it decodes to."""
    from otvm_amd import engine
    from otvm_amd.synth_data import synthetic_clip
    from tests.test_gpu_frame import _fresh_model
    d = tmp_path_factory.mktemp("y4m")
    old, old_auto = os.environ.get("OTVM_TUNE_FILE"), engine.AUTOTUNE
    os.environ["OTVM_TUNE_FILE"] = os.path.join(str(d), "tune.json")
    engine.AUTOTUNE = False
    try:
        frames_bgr, tri = synthetic_clip(H_, W_, T_, seed=53)
        path = os.path.join(str(d), "clip.y4m")
        yield _fresh_model(synth_sd, 12, "f16x3"), path, _write_clip(path, frames_bgr), tri
    finally:
        engine.AUTOTUNE = old_auto
        if old is None:
            os.environ.pop("OTVM_TUNE_FILE", None)
        else:
            os.environ["OTVM_TUNE_FILE"] = old


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_y4m_frames_are_prefetched_frames(route):
    from otvm_amd import yuv
    _, path, host, _ = route
    src = yuv.Y4MFrames(path, DEV, depth=2)
    assert len(src) == T_ and not hasattr(src, "shape") and (src.matrix, src.range, src.header.siting) == ("601", "limited", "left")
    for i in (0, 1, 2, 3, 1, 0, 3):                                                   # forward, backward, a jump
        d = src[i]
        assert d.dtype == torch.uint8 and tuple(d.shape) == (H_, W_, 3) and d.device == torch.device(DEV)
        d._otvm_ready.synchronize()
        assert np.array_equal(d.cpu().numpy(), host[i]), i
    with pytest.raises(IndexError):
        src[T_]
    src.close()
    bgr = yuv.Y4MFrames(path, DEV, order="bgr")
    d = bgr[2]
    d._otvm_ready.synchronize()
    assert np.array_equal(d.cpu().numpy(), host[2][..., ::-1])
    bgr.close()


@pytest.mark.parametrize("case", ["plain", "work_scale", "stabilise", "keyframes"])
def test_run_video_matte_from_y4m_equals_the_run_on_host_arrays(route, case):
    from otvm_amd import yuv
    from otvm_amd.video import run_video_matte
    m, path, host, tri = route
    kw = {"plain": dict(trimap=tri), "work_scale": dict(trimap=tri, work_scale=2), "stabilise": dict(trimap=tri, stabilise=True),
          "keyframes": dict(keyframes={0: tri, 3: tri})}[case]
    src = yuv.Y4MFrames(path, DEV)
    got = run_video_matte(m, src, **RUN, **kw)
    src.close()
    want = run_video_matte(m, host, **RUN, **kw)
    for k in ("alpha", "alpha_u8", "trimap"):
        assert _eq(got[k], want[k]), k
    assert got["bank_frames"] == want["bank_frames"]
    if case == "keyframes":
        order = [s[0] for s in got["schedule"]]
        assert order != sorted(order)                                                 # a backward sweep: random access was used


def _parse_stream(data, nbytes):
    from otvm_amd import yuv
    h = yuv.parse_y4m_header(data)
    body, frames = data[h.length:], []
    assert len(body) % (6 + nbytes) == 0
    for k in range(len(body) // (6 + nbytes)):
        chunk = body[k * (6 + nbytes):(k + 1) * (6 + nbytes)]
        assert chunk[:6] == b"FRAME\n"
        frames.append(chunk[6:])
    return h, frames


def test_writer_streams_equal_the_restatement(route, tmp_path):
    from otvm_amd import yuv
    from otvm_amd.video import run_video_matte
    m, path, host, tri = route
    res = run_video_matte(m, host, trimap=tri, new_background=(0, 255, 0), keep_on_device=True, **RUN)
    sink = io.BytesIO()
    aw = yuv.Y4MWriter(sink, DEV, W_, H_, rate="25:1", kind="mono", depth=2)
    cpath = str(tmp_path / "comp.y4m")
    cw = yuv.Y4MWriter(cpath, DEV, W_, H_, rate="25:1", kind="420", depth=2)
    for t in range(T_):
        aw.put(t, res["alpha_u8"][t])
        cw.put(t, res["comp_u8"][t])
    with pytest.raises(ValueError, match="order"):
        aw.put(T_ + 1, res["alpha_u8"][0])
    with pytest.raises(ValueError, match="order"):
        cw.put(0, res["comp_u8"][0])
    with pytest.raises(ValueError):
        aw.put(T_, res["comp_u8"][0])                                                  # [H,W,3] into a mono stream
    aw.close()
    cw.close()
    h, frames = _parse_stream(sink.getvalue(), H_ * W_)
    assert (h.W, h.H, h.F, h.C, h.full_range) == (W_, H_, "25:1", "mono", True) and len(frames) == T_
    for t in range(T_):
        assert frames[t] == res["alpha_u8"][t].cpu().numpy().tobytes(), t
    h, frames = _parse_stream(open(cpath, "rb").read(), yuv.frame_bytes(H_, W_, "420p"))
    assert (h.C, h.full_range) == ("420jpeg", False) and len(frames) == T_
    for t in range(T_):
        assert frames[t] == R.pack_frame(*R.rgb_to_yuv420(res["comp_u8"][t].cpu().numpy(), "601", "limited", rgb=True)), t


def test_y4m_cli_end_to_end(route, tmp_path):
    from PIL import Image
    from otvm_amd import yuv
    from otvm_amd.video import run_video_matte
    m, path, host, tri = route
    tpng = str(tmp_path / "trimap.png")
    Image.fromarray((tri[1] * 128 + tri[2] * 255).astype(np.uint8)).save(tpng)
    apath, cpath = str(tmp_path / "alpha.y4m"), str(tmp_path / "comp.y4m")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["OTVM_AUTOTUNE"] = "0"                                                        # as the fixture's engine.AUTOTUNE = False
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "otvm_amd.y4m_cli", path, "--trimap", tpng, "--alpha", apath, "--comp", cpath, "--composite",
                        "0,255,0", "--synthetic-weights", "--skip", "2", "--max-num", "3"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["frames"] == T_ and (summary["width"], summary["height"]) == (W_, H_) and summary["fps"] > 0
    assert summary["chroma"] == "C420mpeg2" and summary["matrix"] == "601" and summary["range"] == "limited"
    ha, alphas = _parse_stream(open(apath, "rb").read(), H_ * W_)
    hc, comps = _parse_stream(open(cpath, "rb").read(), yuv.frame_bytes(H_, W_, "420p"))
    assert (ha.W, ha.H, ha.C, ha.F, len(alphas)) == (W_, H_, "mono", "25:1", T_)
    assert (hc.W, hc.H, hc.C, len(comps)) == (W_, H_, "420jpeg", T_)
    src = yuv.Y4MFrames(path, DEV)
    ref = run_video_matte(m, src, trimap=tri, new_background=(0, 255, 0), **RUN)
    src.close()
    for t in range(T_):
        assert alphas[t] == ref["alpha_u8"][t].numpy().tobytes(), t
        assert comps[t] == R.pack_frame(*R.rgb_to_yuv420(ref["comp_u8"][t].numpy(), "601", "limited", rgb=True)), t
