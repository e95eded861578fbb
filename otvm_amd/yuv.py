"""Video streams: Y4M (YUV4MPEG2) in and out, YUV <-> RGB on the device (include/otvm_hip.h: otvm_yuv_to_rgb, otvm_rgb_to_yuv420).

Footage leaves a decoder as 8-bit YUV, usually 4:2:0 and limited range, and ``ffmpeg ... -f yuv4mpegpipe`` is the usual glue between
tools.  This module is a frame SOURCE and a frame SINK for ``run_video_matte`` -- the driver itself is unchanged:

  * ``Y4MFrames`` reads a Y4M file or pipe, one reader thread filling pinned host buffers ahead; ``frames[i]`` uploads the frame as
    it lies in the file (1.5 bytes a pixel for 4:2:0, no host decode), converts it to uint8 [H,W,3] with one launch on the source's
    copy stream, and returns that tensor carrying the event behind both as ``_otvm_ready`` -- to the driver it is a prefetched PNG
    frame (io_pipeline.FramePrefetcher).  Pass ``frames_are_rgb=True`` (order="rgb", the default).
  * ``Y4MWriter`` takes the 8-bit alphas (``kind="mono"``: a ``Cmono`` full-range stream of the bytes as they are) or composites
    (``kind="420"``: otvm_rgb_to_yuv420 on the caller's stream, labelled ``C420jpeg``), downloads on a copy stream into pinned
    memory, and one writer thread emits the frames in index order.
  * ``yuv_to_rgb`` / ``rgb_to_yuv420`` are the two launches alone, for callers whose planes never were Y4M (NV12 surfaces).

The conversion is CHECKED BY DEFINITION ONLY: integer arithmetic within one code value of bilinear chroma at the stated siting, the
standard's matrix, round half up, clamp (tests/yuv_ref.py).  A Y4M header does not carry the matrix: ``matrix="auto"`` takes BT.709
when H >= 720 and BT.601 below, which is a CONVENTION of the tools that write such files, not a measurement of the footage.

Refused: ``C420paldv``, every high-bit-depth tag (``...p10``, ``p12``, ``p16``), alpha-carrying tags (``C444alpha``) and interlaced
streams (``It``, ``Ib``, ``Im``).
"""
import ctypes as C
import os
import queue
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import lib as L

MAGIC = b"YUV4MPEG2"
# chroma tag (without the leading C) -> (layout, horizontal chroma siting)
CHROMA_TAGS = {"420jpeg": ("420p", "centre"), "420mpeg2": ("420p", "left"), "420": ("420p", "left"), "422": ("422p", "left"),
               "444": ("444p", "left"), "mono": ("mono", "left")}
LAYOUTS = {"420p": L.YUV_420P, "nv12": L.YUV_NV12, "422p": L.YUV_422P, "444p": L.YUV_444P, "mono": L.YUV_MONO}
MATRICES = {"601": L.YUV_BT601, "709": L.YUV_BT709}
RANGES = {"limited": L.YUV_LIMITED, "full": L.YUV_FULL}
SITINGS = {"left": L.YUV_SITING_LEFT, "centre": L.YUV_SITING_CENTRE}


class Y4MError(ValueError):
    pass


class Y4MHeader:
    """The stream header: W, H, F (rate "num:den"), I (interlacing, only "p"), A (pixel aspect "num:den" or None), C (the chroma tag
    without its leading C) and full_range (XCOLORRANGE=FULL; limited when the header does not say).  ``length`` is the number of
    bytes the header line took, its newline included (0 for a header made by hand)."""

    def __init__(self, W, H, F="30:1", I="p", A=None, C="420jpeg", full_range=False, length=0):
        self.W, self.H, self.F, self.I, self.A, self.C, self.full_range, self.length = int(W), int(H), F, I, A, C, bool(full_range), length
        check_header(self)

    def __eq__(self, o):
        return isinstance(o, Y4MHeader) and self.fields() == o.fields()

    def __repr__(self):
        return "Y4MHeader(%s)" % ", ".join("%s=%r" % kv for kv in self.fields())

    def fields(self):
        return (("W", self.W), ("H", self.H), ("F", self.F), ("I", self.I), ("A", self.A), ("C", self.C), ("full_range", self.full_range))

    @property
    def layout(self):
        return CHROMA_TAGS[self.C][0]

    @property
    def siting(self):
        return CHROMA_TAGS[self.C][1]

    @property
    def frame_bytes(self):
        return frame_bytes(self.H, self.W, self.layout)

    @property
    def rate(self):
        num, den = self.F.split(":")
        return int(num) / max(1, int(den))


def check_header(h):
    if h.W < 1 or h.H < 1:
        raise Y4MError("Y4M: the frame size is %d x %d" % (h.W, h.H))
    if h.I in ("t", "b", "m"):
        raise Y4MError("Y4M: interlaced streams are not supported (I%s); deinterlace first" % h.I)
    if h.I not in ("p", "?"):
        raise Y4MError("Y4M: unknown interlacing tag I%s" % h.I)
    tag = h.C
    if tag not in CHROMA_TAGS:
        if tag == "420paldv":
            why = "its chroma siting (PAL DV) is not supported"
        elif "alpha" in tag:
            why = "alpha-carrying streams are not supported"
        elif tag[-3:] in ("p10", "p12", "p14", "p16") or tag[-2:] in ("p9",) or tag in ("mono9", "mono10", "mono12", "mono16"):
            why = "only 8-bit streams are supported"
        else:
            why = "unknown chroma tag"
        raise Y4MError("Y4M: C%s: %s" % (tag, why))


def parse_y4m_header(data):
    """The header line of a Y4M stream (bytes that begin with it; anything after the first newline is not looked at)."""
    data = bytes(data)
    end = data.find(b"\n")
    line = data if end < 0 else data[:end]
    parts = line.split(b" ")
    if parts[0] != MAGIC:
        raise Y4MError("Y4M: the stream does not begin with %s" % MAGIC.decode())
    kw = {}
    for p in parts[1:]:
        if not p:
            continue
        key, val = chr(p[0]), p[1:].decode("ascii", "replace")
        if key in "WHFIAC":
            kw[key] = val
        elif key == "X" and val.startswith("COLORRANGE="):
            r = val[len("COLORRANGE="):]
            if r not in ("FULL", "LIMITED"):
                raise Y4MError("Y4M: XCOLORRANGE=%s is neither FULL nor LIMITED" % r)
            kw["full_range"] = r == "FULL"
    if "W" not in kw or "H" not in kw:
        raise Y4MError("Y4M: the header carries no W / H")
    try:
        W, H = int(kw.pop("W")), int(kw.pop("H"))
    except ValueError:
        raise Y4MError("Y4M: W / H are not numbers")
    if kw.get("A") in ("0:0",):
        kw["A"] = None                                 # "unknown"
    return Y4MHeader(W, H, length=len(line) + (1 if end >= 0 else 0), **kw)


def format_y4m_header(W, H, F="30:1", I="p", A=None, C="420jpeg", full_range=False):
    """The header line, newline included, of a stream parse_y4m_header reads back to the same fields."""
    h = Y4MHeader(W, H, F, I, A, C, full_range)
    parts = [MAGIC.decode(), "W%d" % h.W, "H%d" % h.H, "F%s" % h.F, "I%s" % h.I]
    if h.A:
        parts.append("A%s" % h.A)
    parts += ["C%s" % h.C, "XCOLORRANGE=%s" % ("FULL" if h.full_range else "LIMITED")]
    return (" ".join(parts) + "\n").encode("ascii")


def frame_planes(H, W, layout):
    """[(offset, rows, row bytes)] of the planes of one contiguous frame: Y, then U and V (or the one UV plane of NV12)."""
    cw, ch = (W + 1) // 2, (H + 1) // 2
    shapes = {"420p": [(H, W), (ch, cw), (ch, cw)], "nv12": [(H, W), (ch, 2 * cw)], "422p": [(H, W), (H, cw), (H, cw)],
              "444p": [(H, W)] * 3, "mono": [(H, W)]}[layout]
    out, off = [], 0
    for r, c in shapes:
        out.append((off, r, c))
        off += r * c
    return out


def frame_bytes(H, W, layout):
    off, r, c = frame_planes(H, W, layout)[-1]
    return off + r * c


def resolve_matrix(matrix, H):
    """"auto": BT.709 at H >= 720, BT.601 below -- a convention, not a measurement; "601" / "709" as given."""
    m = str(matrix)
    if m == "auto":
        return "709" if H >= 720 else "601"
    if m not in MATRICES:
        raise ValueError("matrix is auto, 601 or 709, got %r" % (matrix,))
    return m


def _resolve_range(rng, header_full):
    if rng is None:
        return "full" if header_full else "limited"
    if rng not in RANGES:
        raise ValueError("range is limited, full or None (the header's), got %r" % (rng,))
    return rng


def _order_flag(order):
    if order not in ("rgb", "bgr"):
        raise ValueError("order is rgb or bgr, got %r" % (order,))
    return int(order == "rgb")


class Y4MReader:
    """The container alone, no device: the header, the number of frames and ``read_into(i, buffer)``.  On a seekable file T comes
    from the file's size and any frame can be read; on a pipe ``frames`` is required and the frames come in order."""

    def __init__(self, path_or_file, frames=None):
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike))
        if self._own:
            self.f = sys.stdin.buffer if path_or_file == "-" else open(path_or_file, "rb")
            self._own = path_or_file != "-"
        else:
            self.f = path_or_file
        line = self.f.readline(4096)
        self.header = parse_y4m_header(line)
        if not line.endswith(b"\n"):
            raise Y4MError("Y4M: the header line does not end")
        self.nbytes = self.header.frame_bytes
        try:
            self.seekable = bool(self.f.seekable())
        except (AttributeError, OSError):
            self.seekable = False
        self._pos = 0                                      # pipes: the next frame in the stream
        if self.seekable:
            self._offsets = self._index(len(line))
            self.T = len(self._offsets) if frames is None else min(int(frames), len(self._offsets))
            if frames is not None and int(frames) > len(self._offsets):
                raise Y4MError("Y4M: the stream ends before frame %d (%d frames asked for)" % (len(self._offsets), int(frames)))
        else:
            if frames is None:
                raise ValueError("Y4M: a pipe does not say how long it is: pass frames=N")
            self.T = int(frames)

    def _index(self, start):
        """Offsets of every frame's data.  Plain ``FRAME\\n`` markers (the usual case): from the file's size alone; a stream whose
        markers carry parameters is walked once, marker by marker."""
        f = self.f
        size = f.seek(0, os.SEEK_END)
        f.seek(start)
        step = 6 + self.nbytes
        first = f.readline(4096)
        if first == b"":
            return []
        if first == b"FRAME\n" and (size - start) % step == 0:
            return [start + 6 + k * step for k in range((size - start) // step)]
        offs, pos = [], start
        while pos < size:
            f.seek(pos)
            line = f.readline(4096)
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise Y4MError("Y4M: no FRAME marker where frame %d should begin (byte %d)" % (len(offs), pos))
            if pos + len(line) + self.nbytes > size:
                raise Y4MError("Y4M: the stream ends inside frame %d" % len(offs))
            offs.append(pos + len(line))
            pos += len(line) + self.nbytes
        return offs

    def read_into(self, i, buf):
        """Frame ``i``'s bytes into ``buf`` (a writable buffer of nbytes)."""
        f = self.f
        if self.seekable:
            if not 0 <= i < self.T:
                raise IndexError("Y4M: frame %d of %d" % (i, self.T))
            f.seek(self._offsets[i] - 6)
            if f.read(6)[-1:] != b"\n":
                raise Y4MError("Y4M: no FRAME marker in front of frame %d" % i)
        else:
            if i != self._pos:
                raise Y4MError("Y4M: a pipe is read in order: frame %d asked for, frame %d is next" % (i, self._pos))
            line = f.readline(4096)
            if line == b"":
                raise Y4MError("Y4M: the stream ends before frame %d (%d frames asked for)" % (i, self.T))
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise Y4MError("Y4M: no FRAME marker where frame %d should begin" % i)
            self._pos += 1
        view, got = memoryview(buf).cast("B"), 0
        while got < self.nbytes:
            n = f.readinto(view[got:self.nbytes])
            if not n:
                raise Y4MError("Y4M: the stream ends inside frame %d (%d of %d bytes)" % (i, got, self.nbytes))
            got += n

    def close(self):
        if self._own:
            self.f.close()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _launch_to_rgb(buf, H, W, layout, matrix, rng, siting, u8_rgb, out, stream, planes=None, strides=None):
    """One otvm_yuv_to_rgb launch on the planes of the contiguous frame ``buf`` (or on ``planes`` = data pointers, ``strides``)."""
    if planes is None:
        geo = frame_planes(H, W, layout)
        base = buf.data_ptr()
        planes = [base + o for o, _, _ in geo] + [0, 0]
        strides = [c for _, _, c in geo] + [0, 0]
    p = L.YuvToRgbParams(H=H, W=W, layout=LAYOUTS[layout], matrix=MATRICES[matrix], range=RANGES[rng], siting=SITINGS[siting],
                         y_stride=strides[0], u_stride=strides[1], v_stride=strides[2], u8_rgb=u8_rgb,
                         y=planes[0], u=planes[1] or None, v=planes[2] or None, rgb=out.data_ptr())
    L.check(L.load().otvm_yuv_to_rgb(C.byref(p), stream), "yuv_to_rgb")


def _launch_to_yuv420(img, H, W, matrix, rng, u8_rgb, buf, stream):
    geo = frame_planes(H, W, "420p")
    base = buf.data_ptr()
    p = L.RgbToYuv420Params(H=H, W=W, matrix=MATRICES[matrix], range=RANGES[rng], y_stride=geo[0][2], u_stride=geo[1][2],
                            v_stride=geo[2][2], u8_rgb=u8_rgb, img=img.data_ptr(), y=base + geo[0][0], u=base + geo[1][0],
                            v=base + geo[2][0])
    L.check(L.load().otvm_rgb_to_yuv420(C.byref(p), stream), "rgb_to_yuv420")


def _u8_plane(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.stride(-1) == 1 and (t.dim() == 2 or (t.dim() == 3 and t.stride(1) == t.shape[2]))):
        raise ValueError("yuv_to_rgb: %s is a uint8 device tensor with contiguous rows" % what)
    return t


def yuv_to_rgb(y, u=None, v=None, layout="420p", matrix="auto", range="limited", siting="left", order="rgb", out=None):
    """Device planes -> uint8 [H,W,3] on the current stream.  y [H,W]; u, v as the layout says (nv12: u is [ch,cw,2], v None; mono:
    neither); a plane may be a view with a row stride of its own (rows themselves contiguous)."""
    _u8_plane(y, "y")
    H, W = y.shape
    planes, strides = [y.data_ptr(), 0, 0], [y.stride(0), 0, 0]
    want = {"420p": 2, "nv12": 1, "422p": 2, "444p": 2, "mono": 0}[layout]
    cw, ch = (W + 1) // 2, (H + 1) // 2
    shape = {"420p": (ch, cw), "nv12": (ch, cw, 2), "422p": (H, cw), "444p": (H, W), "mono": None}[layout]
    for k, t in enumerate((u, v)[:want]):
        _u8_plane(t, "uv"[k])
        if tuple(t.shape) != shape:
            raise ValueError("yuv_to_rgb: the %s plane of a %dx%d %s frame is %s, got %s" % ("uv"[k], W, H, layout, shape, tuple(t.shape)))
        planes[1 + k], strides[1 + k] = t.data_ptr(), t.stride(0)
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=y.device)
    _launch_to_rgb(None, H, W, layout, resolve_matrix(matrix, H), range, siting, _order_flag(order), out, _stream(y.device), planes, strides)
    return out


def rgb_to_yuv420(img, matrix="auto", range="limited", order="rgb", out=None):
    """uint8 [H,W,3] on the device -> (frame, (y, u, v)): one contiguous planar 4:2:0 frame (centre-sited chroma, "C420jpeg") and
    views of its planes, on the current stream."""
    if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.is_contiguous()):
        raise ValueError("rgb_to_yuv420: img is a contiguous uint8 [H,W,3] device tensor")
    H, W = img.shape[:2]
    n = frame_bytes(H, W, "420p")
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=img.device)
    _launch_to_yuv420(img, H, W, resolve_matrix(matrix, H), range, _order_flag(order), out, _stream(img.device))
    views = tuple(out[o:o + r * c].view(r, c) for o, r, c in frame_planes(H, W, "420p"))
    return out, views


class Y4MFrames:
    """A Y4M file or pipe as the ``frames`` of run_video_matte: len(), ``frames[i]`` -> uint8 [H,W,3] on the device with
    ``_otvm_ready`` (the event behind the upload and the conversion, both on this source's copy stream).  One reader thread
    fills pinned buffers ``depth`` frames ahead in the direction of the last two requests, so the backward sweep of a keyframe
    schedule is read ahead too (seekable files; a pipe is read in order and needs ``frames=N``).  ``matrix="auto"`` is a
    convention (resolve_matrix), ``range=None`` the header's."""

    def __init__(self, path_or_file, device, depth=6, order="rgb", matrix="auto", range=None, frames=None):
        self.reader = Y4MReader(path_or_file, frames)
        h = self.header = self.reader.header
        self.dev = torch.device(device)
        self.depth = max(1, int(depth))
        self.u8_rgb = _order_flag(order)
        self.matrix, self.range = resolve_matrix(matrix, h.H), _resolve_range(range, h.full_range)
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.pool = ThreadPoolExecutor(max_workers=1)      # ONE reader: the file has one position
        self._futs, self._last = {}, None

    def __len__(self):
        return self.reader.T

    @property
    def rereadable(self):
        """Whether a frame can be asked for a second time (a seekable file; not a pipe): what a pre-pass over the clip needs"""
        return self.reader.seekable

    def _load(self, i):
        host = torch.empty(self.reader.nbytes, dtype=torch.uint8, pin_memory=True)
        self.reader.read_into(i, host.numpy())             # straight into the pinned staging buffer
        return host

    def _schedule(self, i):
        T = self.reader.T
        step = -1 if (self.reader.seekable and self._last is not None and i < self._last) else 1
        want = [j for j in (i + step * k for k in range(self.depth)) if 0 <= j < T]
        if self.reader.seekable:
            for j in [j for j in self._futs if j not in want]:
                self._futs.pop(j).cancel()                 # read ahead for a sweep that turned: not needed any more
        for j in want:
            if j not in self._futs:
                self._futs[j] = self.pool.submit(self._load, j)
        self._last = i

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < self.reader.T:
            raise IndexError("Y4M: frame %d of %d" % (i, self.reader.T))
        self._schedule(i)
        host = self._futs.pop(i).result()
        h = self.header
        with torch.cuda.stream(self.copy_stream):
            buf = host.to(self.dev, non_blocking=True)
            rgb = torch.empty((h.H, h.W, 3), dtype=torch.uint8, device=self.dev)
            _launch_to_rgb(buf, h.H, h.W, h.layout, self.matrix, self.range, h.siting, self.u8_rgb, rgb, self.copy_stream.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        # as FramePrefetcher: the consumer waits for the event itself (run_video_matte hands it to the model as _inputs_ready)
        rgb.record_stream(torch.cuda.current_stream(self.dev))
        rgb._otvm_ready = ev
        return rgb

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)
        self.reader.close()


class Y4MWriter:
    """Asynchronous Y4M sink.  ``put(i, u8)``: kind="mono" takes the alpha bytes [H,W] as they are (``Cmono``,
    XCOLORRANGE=FULL, no kernel); kind="420" takes [H,W,3] and runs otvm_rgb_to_yuv420 on the caller's stream into a device frame
    (``C420jpeg``).  The download runs on a copy stream into pinned memory and ONE writer thread emits ``FRAME`` plus the bytes,
    so frames must be put in index order -- a natural-order schedule; a keyframe clip with a backward sweep has none.  The queue
    holds ``depth`` frames: put() blocks when the sink is slower than the device."""

    def __init__(self, path_or_file, device, W, H, rate="30:1", kind="mono", matrix="auto", range="limited", depth=8, order="rgb"):
        if kind not in ("mono", "420"):
            raise ValueError("Y4MWriter: kind is mono or 420, got %r" % (kind,))
        self.dev, self.W, self.H, self.kind = torch.device(device), int(W), int(H), kind
        self.u8_rgb = _order_flag(order)
        self.matrix = resolve_matrix(matrix, self.H)
        self.range = "full" if kind == "mono" else _resolve_range(range, False)
        self.layout = "mono" if kind == "mono" else "420p"
        self.nbytes = frame_bytes(self.H, self.W, self.layout)
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike)) and path_or_file != "-"
        self.f = sys.stdout.buffer if path_or_file == "-" else open(path_or_file, "wb") if self._own else path_or_file
        self.f.write(format_y4m_header(self.W, self.H, rate, C="mono" if kind == "mono" else "420jpeg", full_range=self.range == "full"))
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.q = queue.Queue(maxsize=max(1, int(depth)))
        self._next, self._err, self._closed = 0, None, False
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            if self._err is not None:
                continue                                   # keep draining, so that no put() blocks for ever
            try:
                host, done = item
                done.synchronize()
                self.f.write(b"FRAME\n")
                self.f.write(memoryview(host.numpy()))
            except Exception as e:                          # reported by the next put() / close()
                self._err = e

    def put(self, i, u8):
        if self._err is not None:
            raise self._err
        if self._closed:
            raise ValueError("Y4MWriter: put() after close()")
        if i != self._next:
            raise ValueError("Y4MWriter: frame %d put where frame %d is due: a Y4M stream is written in index order (a natural-order "
                             "schedule, no backward sweep)" % (i, self._next))
        shape = (self.H, self.W) if self.kind == "mono" else (self.H, self.W, 3)
        if tuple(u8.shape) != shape or u8.dtype != torch.uint8:
            raise ValueError("Y4MWriter: kind=%s takes uint8 %s, got %s %s" % (self.kind, shape, u8.dtype, tuple(u8.shape)))
        cur = torch.cuda.current_stream(self.dev)
        if self.kind == "mono":
            src = u8.contiguous()
        else:
            src = torch.empty(self.nbytes, dtype=torch.uint8, device=self.dev)
            _launch_to_yuv420(u8.contiguous(), self.H, self.W, self.matrix, self.range, self.u8_rgb, src, cur.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(cur)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ev)
            host = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
            host.copy_(src.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        src.record_stream(self.copy_stream)
        self._next += 1
        self.q.put((host, done))

    def close(self):
        if not self._closed:
            self._closed = True
            self.q.put(None)
            self.thread.join()
            self.f.flush()
            if self._own:
                self.f.close()
        if self._err is not None:
            raise self._err
