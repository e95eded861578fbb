"""Video streams without a GPU: the numpy restatement of otvm_yuv_to_rgb / otvm_rgb_to_yuv420 (tests/yuv_ref.py) against their
float64 definition, the grey property, the Y4M container (otvm_amd/yuv.py: header, frame sizes, framing, refusals) and the
declarations of the new symbols.  The bound of one code value is derived in tests/yuv_ref.py's docstring."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests import yuv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 2), (3, 5), (7, 9), (33, 65)]
MATRICES, RANGES = ("601", "709"), ("limited", "full")


def sitings(layout):
    return ("left", "centre") if R.SUBSAMPLING[layout][0] else ("left",)


# ------------------------------------------------------------------------------------------------ restatement against definition
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_yuv_to_rgb_restatement_is_within_one_of_the_definition(layout):
    rng_ = np.random.default_rng(7)
    worst = 0
    for H, W in SIZES:
        for corners in (False, True):
            y, u, v = R.random_planes(rng_, H, W, layout, corners)
            for siting in sitings(layout):
                for matrix in MATRICES:
                    for rng in RANGES:
                        for rgb in (True, False):
                            got = R.yuv_to_rgb(y, u, v, layout, matrix, rng, siting, rgb).astype(int)
                            want = R.yuv_to_rgb_definition(y, u, v, layout, matrix, rng, siting, rgb).astype(int)
                            assert got.shape == (H, W, 3)
                            worst = max(worst, int(np.abs(got - want).max()))
                            assert np.abs(got - want).max() <= 1, (layout, H, W, siting, matrix, rng)
    print("yuv_to_rgb %s: max |restatement - definition| = %d" % (layout, worst))


def test_rgb_to_yuv420_restatement_is_within_one_of_the_definition():
    rng_ = np.random.default_rng(11)
    for H, W in SIZES:
        for corners in (False, True):
            img = (rng_.choice(np.array([0, 16, 128, 235, 240, 255], np.uint8), size=(H, W, 3)) if corners
                   else rng_.integers(0, 256, (H, W, 3), dtype=np.uint8))
            for matrix in MATRICES:
                for rng in RANGES:
                    for rgb in (True, False):
                        got = R.rgb_to_yuv420(img, matrix, rng, rgb)
                        want = R.rgb_to_yuv420_definition(img, matrix, rng, rgb)
                        for g, w, shape in zip(got, want, [(H, W)] + [((H + 1) // 2, (W + 1) // 2)] * 2):
                            assert g.shape == shape and g.dtype == np.uint8
                            assert np.abs(g.astype(int) - w.astype(int)).max() <= 1, (H, W, matrix, rng)


def test_chroma_taps_are_the_stated_rule():
    c = np.array([[10, 50, 90]], np.uint8)                                             # one chroma row, W = 6 (4:2:2)
    centre = R.chroma16(c, 1, 6, "422p", "centre")[0] // 4
    left = R.chroma16(c, 1, 6, "422p", "left")[0] // 4
    assert centre.tolist() == [4 * 10, 3 * 10 + 50, 3 * 50 + 10, 3 * 50 + 90, 3 * 90 + 50, 4 * 90]
    assert left.tolist() == [4 * 10, 2 * 10 + 2 * 50, 4 * 50, 2 * 50 + 2 * 90, 4 * 90, 4 * 90]
    col = np.array([[10], [50]], np.uint8)                                             # 4:2:0 rows: the centre rule, H = 4
    assert (R.chroma16(col, 4, 1, "420p", "left")[:, 0] // 4).tolist() == [4 * 10, 3 * 10 + 50, 3 * 50 + 10, 4 * 50]
    assert (R.chroma16(c, 1, 3, "444p", "left")[0]).tolist() == [160, 800, 1440]


def test_constants_are_exact_where_they_must_be():
    for matrix in MATRICES:
        for rng in RANGES:
            yr, yg, yb, ch, ur, vb = R.forward_constants(matrix, rng)
            cy = R.inverse_constants(matrix, rng)[0]
            assert min(yr, yg, yb, ch, ur, vb, ch - ur, ch - vb) > 0
            if rng == "full":
                assert yr + yg + yb == 1 << R.SHIFT and cy == 1 << R.SHIFT and ch == 1 << (R.SHIFT - 1)
            else:
                assert yr + yg + yb == round(219 / 255 * (1 << R.SHIFT))
            # the chroma rows (-UR, -(CH - UR), CH) and (CH, -(CH - VB), -VB) sum to zero by construction
            assert -ur - (ch - ur) + ch == 0 and ch - (ch - vb) - vb == 0


def test_grey_is_grey_exactly_in_full_range():
    v = np.arange(256, dtype=np.uint8)
    img = np.repeat(v.reshape(16, 16, 1), 3, axis=2)
    for matrix in MATRICES:
        y, u, vv = R.rgb_to_yuv420(img, matrix, "full")
        assert np.array_equal(y, img[..., 0]) and (u == 128).all() and (vv == 128).all()
        for layout in R.LAYOUTS:
            ch, cw = R.chroma_shape(16, 16, layout)
            c = None if layout == "mono" else np.full((ch, cw, 2) if layout == "nv12" else (ch, cw), 128, np.uint8)
            for siting in sitings(layout):
                back = R.yuv_to_rgb(img[..., 0], c, c, layout, matrix, "full", siting)
                assert np.array_equal(back, img), (matrix, layout, siting)


def test_kernel_source_and_header_carry_the_restatements_integers():
    src = open(os.path.join(ROOT, "otvm_amd", "csrc", "yuv.hip")).read()
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    for matrix in MATRICES:
        for rng in RANGES:
            for consts in (R.inverse_constants(matrix, rng), R.forward_constants(matrix, rng)):
                lit = ", ".join(str(c) for c in consts)
                assert "{%s}" % lit in src, (matrix, rng, lit)
                assert lit in header, (matrix, rng, lit)


# ------------------------------------------------------------------------------------------------ the container
def test_header_round_trip_and_defaults():
    from otvm_amd import yuv
    for kw in (dict(W=1920, H=1080, F="30000:1001", A="1:1", C="420mpeg2", full_range=False),
               dict(W=3, H=5, F="25:1", C="444", full_range=True), dict(W=150, H=100, C="mono", full_range=True),
               dict(W=7, H=9, C="422"), dict(W=8, H=8, C="420jpeg"), dict(W=8, H=8, C="420")):
        line = yuv.format_y4m_header(**kw)
        assert line.startswith(b"YUV4MPEG2 ") and line.endswith(b"\n")
        h = yuv.parse_y4m_header(line + b"FRAME\n")
        assert h == yuv.Y4MHeader(**kw) and h.length == len(line)
        assert yuv.parse_y4m_header(yuv.format_y4m_header(h.W, h.H, h.F, h.I, h.A, h.C, h.full_range)) == h
    h = yuv.parse_y4m_header(b"YUV4MPEG2 W4 H6 F24:1\n")
    assert (h.W, h.H, h.F, h.I, h.C, h.full_range, h.layout, h.siting) == (4, 6, "24:1", "p", "420jpeg", False, "420p", "centre")
    assert yuv.parse_y4m_header(b"YUV4MPEG2 W4 H6 C420\n").siting == "left" and yuv.parse_y4m_header(b"YUV4MPEG2 W4 H6 C420mpeg2\n").siting == "left"
    assert yuv.parse_y4m_header(b"YUV4MPEG2 W4 H6 XCOLORRANGE=FULL XYSCSS=420JPEG\n").full_range is True
    assert abs(yuv.parse_y4m_header(b"YUV4MPEG2 W4 H6 F30000:1001\n").rate - 29.97) < 0.01
    assert yuv.resolve_matrix("auto", 720) == "709" and yuv.resolve_matrix("auto", 719) == "601" and yuv.resolve_matrix("601", 2160) == "601"
    with pytest.raises(ValueError):
        yuv.resolve_matrix("2020", 100)


@pytest.mark.parametrize("tag", ["C420paldv", "C420p10", "C422p10", "C444p12", "C444p16", "C420p16", "Cmono16", "C444alpha", "It", "Ib", "Im"])
def test_header_refusals_name_the_tag(tag):
    from otvm_amd import yuv
    with pytest.raises(yuv.Y4MError, match=re.escape(tag)):
        yuv.parse_y4m_header(b"YUV4MPEG2 W4 H6 F24:1 " + tag.encode() + b"\n")


def test_header_refusals_of_malformed_streams():
    from otvm_amd import yuv
    for bad in (b"RIFF W4 H6\n", b"YUV4MPEG2 H6\n", b"YUV4MPEG2 W0 H6\n", b"YUV4MPEG2 W4 H6 Cwhatever\n", b"YUV4MPEG2 W4 H6 XCOLORRANGE=WIDE\n"):
        with pytest.raises(yuv.Y4MError):
            yuv.parse_y4m_header(bad)


def test_frame_byte_counts_for_odd_sizes():
    from otvm_amd import yuv
    for H, W in [(1, 1), (3, 5), (7, 9), (100, 150), (1080, 1920)]:
        ch, cw = (H + 1) // 2, (W + 1) // 2
        assert yuv.frame_bytes(H, W, "420p") == H * W + 2 * ch * cw == yuv.frame_bytes(H, W, "nv12")
        assert yuv.frame_bytes(H, W, "422p") == H * W + 2 * H * cw
        assert yuv.frame_bytes(H, W, "444p") == 3 * H * W and yuv.frame_bytes(H, W, "mono") == H * W
        for layout in R.LAYOUTS:
            y, u, v = R.random_planes(np.random.default_rng(1), H, W, layout)
            assert len(R.pack_frame(y, u, v, layout)) == yuv.frame_bytes(H, W, layout)
    assert yuv.frame_planes(3, 5, "420p") == [(0, 3, 5), (15, 2, 3), (21, 2, 3)]
    assert yuv.frame_planes(3, 5, "nv12") == [(0, 3, 5), (15, 2, 6)]
    assert yuv.parse_y4m_header(b"YUV4MPEG2 W5 H3 C420jpeg\n").frame_bytes == 27


def _two_frames(H=3, W=5, tag="420mpeg2", markers=(b"FRAME\n", b"FRAME\n")):
    from otvm_amd import yuv
    layout = yuv.CHROMA_TAGS[tag][0]
    rng_ = np.random.default_rng(5)
    frames = [R.pack_frame(*R.random_planes(rng_, H, W, layout), layout=layout) for _ in markers]
    data = yuv.format_y4m_header(W, H, "25:1", C=tag) + b"".join(m + f for m, f in zip(markers, frames))
    return data, frames


class _Pipe(io.RawIOBase):
    """A stream that cannot seek and hands out at most 7 bytes a read, as a pipe may."""

    def __init__(self, data):
        self.data, self.pos = data, 0

    def readable(self):
        return True

    def seekable(self):
        return False

    def readinto(self, b):
        n = min(len(b), 7, len(self.data) - self.pos)
        b[:n] = self.data[self.pos:self.pos + n]
        self.pos += n
        return n


def _read(reader, i):
    buf = np.zeros(reader.nbytes, np.uint8)
    reader.read_into(i, buf)
    return buf.tobytes()


def test_reader_framing_on_a_file_and_on_a_pipe(tmp_path):
    from otvm_amd import yuv
    data, frames = _two_frames()
    path = str(tmp_path / "two.y4m")
    open(path, "wb").write(data)
    for src in (path, io.BytesIO(data)):
        r = yuv.Y4MReader(src)
        assert r.seekable and r.T == 2 and r.nbytes == 27 and r.header.C == "420mpeg2"
        assert _read(r, 1) == frames[1] and _read(r, 0) == frames[0] and _read(r, 1) == frames[1]      # random access
        with pytest.raises(IndexError):
            _read(r, 2)
        r.close()
    assert yuv.Y4MReader(path, frames=1).T == 1
    with pytest.raises(yuv.Y4MError, match="frame 2"):
        yuv.Y4MReader(path, frames=3)
    with pytest.raises(ValueError, match="frames=N"):
        yuv.Y4MReader(io.BufferedReader(_Pipe(data)))
    r = yuv.Y4MReader(io.BufferedReader(_Pipe(data)), frames=2)
    assert not r.seekable and r.T == 2
    with pytest.raises(yuv.Y4MError, match="in order"):
        _read(r, 1)
    assert _read(r, 0) == frames[0] and _read(r, 1) == frames[1]


def test_frame_markers_with_parameters_are_tolerated():
    from otvm_amd import yuv
    data, frames = _two_frames(markers=(b"FRAME Ip XFOO=1\n", b"FRAME\n"))
    r = yuv.Y4MReader(io.BytesIO(data))
    assert r.T == 2 and _read(r, 0) == frames[0] and _read(r, 1) == frames[1]
    r = yuv.Y4MReader(io.BufferedReader(_Pipe(data)), frames=2)
    assert _read(r, 0) == frames[0] and _read(r, 1) == frames[1]


def test_a_truncated_stream_raises_and_names_the_frame():
    from otvm_amd import yuv
    data, frames = _two_frames()
    with pytest.raises(yuv.Y4MError, match="frame 1"):
        yuv.Y4MReader(io.BytesIO(data[:-5]))
    r = yuv.Y4MReader(io.BufferedReader(_Pipe(data[:-5])), frames=2)
    assert _read(r, 0) == frames[0]
    with pytest.raises(yuv.Y4MError, match="inside frame 1"):
        _read(r, 1)
    r = yuv.Y4MReader(io.BufferedReader(_Pipe(data[:len(data) - 27 - 6])), frames=2)
    assert _read(r, 0) == frames[0]
    with pytest.raises(yuv.Y4MError, match="before frame 1"):
        _read(r, 1)
    with pytest.raises(yuv.Y4MError, match="FRAME marker"):
        yuv.Y4MReader(io.BytesIO(data[:r.header.length] + b"JUNK!\n" + data[r.header.length + 6:] + b"x"))


# ------------------------------------------------------------------------------------------------ declarations
def test_new_symbols_are_declared_and_the_abi_number_stays():
    from otvm_amd import lib as L
    from otvm_amd.csrc import build
    header = open(os.path.join(ROOT, "include", "otvm_hip.h")).read()
    assert re.search(r"#define OTVM_ABI_VERSION 21\b", header) and L.ABI_VERSION == 21
    assert re.search(r"\bint otvm_yuv_to_rgb\(const otvm_yuv_to_rgb_params\* p, void\* stream\);", header)
    assert re.search(r"\bint otvm_rgb_to_yuv420\(const otvm_rgb_to_yuv420_params\* p, void\* stream\);", header)
    for sym in ("otvm_yuv_to_rgb", "otvm_rgb_to_yuv420"):
        assert sym in L._PROTOS and sym in L.EXPORTED
    assert "yuv.hip" in [s for s, _ in build.SOURCES]
    for name, val in (("420P", L.YUV_420P), ("NV12", L.YUV_NV12), ("422P", L.YUV_422P), ("444P", L.YUV_444P), ("MONO", L.YUV_MONO),
                      ("BT601", L.YUV_BT601), ("BT709", L.YUV_BT709), ("LIMITED", L.YUV_LIMITED), ("FULL", L.YUV_FULL),
                      ("SITING_LEFT", L.YUV_SITING_LEFT), ("SITING_CENTRE", L.YUV_SITING_CENTRE)):
        assert re.search(r"#define OTVM_YUV_%s %d\b" % (name, val), header), name


def test_params_structs_match_the_c_layout(tmp_path):
    """sizeof / offsetof as the C compiler lays the two structs out == the ctypes mirrors, field by field."""
    import shutil
    import subprocess
    from otvm_amd import lib as L
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    for cname, cls in (("otvm_yuv_to_rgb_params", L.YuvToRgbParams), ("otvm_rgb_to_yuv420_params", L.RgbToYuv420Params)):
        names = [n for n, _ in cls._fields_]
        src = ('#include <stdio.h>\n#include <stddef.h>\n#include "otvm_hip.h"\nint main(){printf("%%zu", sizeof(%s));\n' % cname
               + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, n) for n in names) + 'printf("\\n");return 0;}\n')
        exe = str(tmp_path / cname)
        subprocess.run([cc, "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
        got = [int(v) for v in subprocess.check_output([exe]).split()]
        assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in names], cname


def test_library_exports_the_new_symbols_and_refuses_bad_arguments_without_a_device():
    """The built library: ABI 21, both entry points present; every refusal comes from the host side, before any launch, so it is
    testable without a GPU (pointers are never dereferenced on a refusal)."""
    from otvm_amd import lib as L
    lib = L.load()
    assert lib.otvm_abi_version() == 21
    buf = (ctypes.c_ubyte * 64)()
    ptr = ctypes.addressof(buf)

    def to_rgb(**kw):
        base = dict(H=4, W=4, layout=L.YUV_420P, matrix=0, range=0, siting=0, y_stride=4, u_stride=2, v_stride=2, u8_rgb=1, y=ptr, u=ptr,
                    v=ptr, rgb=ptr)
        base.update(kw)
        return L.YuvToRgbParams(**base)

    def to_yuv(**kw):
        base = dict(H=4, W=4, matrix=0, range=0, y_stride=4, u_stride=2, v_stride=2, u8_rgb=1, img=ptr, y=ptr, u=ptr, v=ptr)
        base.update(kw)
        return L.RgbToYuv420Params(**base)

    def refused(rc, name):
        assert rc != 0 and lib.otvm_last_error().decode().startswith(name), lib.otvm_last_error()

    assert lib.otvm_yuv_to_rgb(None, None) != 0 and lib.otvm_rgb_to_yuv420(None, None) != 0
    for kw in (dict(H=0), dict(W=0), dict(H=65536), dict(layout=5), dict(layout=-1), dict(matrix=2), dict(range=2), dict(siting=2),
               dict(y=None), dict(rgb=None), dict(u=None), dict(v=None), dict(y_stride=3), dict(u_stride=1), dict(v_stride=1),
               dict(layout=L.YUV_NV12, u_stride=3), dict(layout=L.YUV_NV12, u=None), dict(layout=L.YUV_444P), dict(layout=L.YUV_422P, u_stride=1)):
        refused(lib.otvm_yuv_to_rgb(ctypes.byref(to_rgb(**kw)), None), "otvm_yuv_to_rgb")
    for kw in (dict(H=0), dict(W=-1), dict(W=65536), dict(matrix=-1), dict(range=7), dict(img=None), dict(y=None), dict(u=None), dict(v=None),
               dict(y_stride=3), dict(u_stride=1), dict(v_stride=0)):
        refused(lib.otvm_rgb_to_yuv420(ctypes.byref(to_yuv(**kw)), None), "otvm_rgb_to_yuv420")
