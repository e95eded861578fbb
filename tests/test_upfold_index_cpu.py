"""CPU: the index / weight helper of the patch conv's upsampled source (otvm_amd/csrc/upfold_index.h) and the ctypes mirror of
otvm_conv_up_params.

The helper is compiled into a stand-alone host program (its own main, -fsanitize=address,undefined) that walks every fine
coordinate of every tile of the shapes tests/test_gpu_upfold.py runs -- the conv's halo included -- and prints the source indices,
the weights and the slots of the tile's source patch.  Checked here against PyTorch's align_corners=False formula restated in numpy."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Hi, Wi) of the source; every shape is walked with the 8-row and the 16-row tile
SHAPES = [(5, 19), (1, 16), (9, 17), (4, 16)]

MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include "upfold_index.h"
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int Hi = atoi(argv[1]), Wi = atoi(argv[2]), TH = atoi(argv[3]);
    const int H = 2 * Hi, W = 2 * Wi, ush = TH == 8 ? otvm_upfold_extent(8) : otvm_upfold_extent(16), usw = otvm_upfold_extent(32);
    // the scratch as the kernel holds it: [ush x usw] slots; every slot the walk names is marked
    unsigned char* scratch = (unsigned char*)malloc((size_t)ush * usw);
    for (int ty0 = 0; ty0 < H; ty0 += TH)
        for (int tx0 = 0; tx0 < W; tx0 += 32) {
            const int sy0 = otvm_upfold_origin(ty0), sx0 = otvm_upfold_origin(tx0);
            memset(scratch, 0, (size_t)ush * usw);
            for (int py = 0; py < TH + 2; ++py)
                for (int px = 0; px < 34; ++px) {
                    const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
                    const OtvmUpAxis ay = otvm_upfold_axis(iy, Hi, sy0, ush), ax = otvm_upfold_axis(ix, Wi, sx0, usw);
                    scratch[ay.s0 * usw + ax.s0] = 1; scratch[ay.s0 * usw + ax.s1] = 1;      // (out of range: the sanitizer stops here)
                    scratch[ay.s1 * usw + ax.s0] = 1; scratch[ay.s1 * usw + ax.s1] = 1;
                    printf("%d %d %d %d %d %d %d %d %u %u %d %d %d %d %d %d %d %d\n", ty0, tx0, iy, ix, ay.i0, ay.i1, ax.i0, ax.i1, bits(ay.l),
                           bits(ax.l), ay.s0, ay.s1, ax.s0, ax.s1, ay.code, ax.code, sy0, sx0);
                }
        }
    free(scratch);
    return 0;
}
"""


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("upfold")
    src, exe = str(d / "upfold_walk.cpp"), str(d / "upfold_walk")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "otvm_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def torch_axis(o, n):
    """area_pixel_compute_source_index(scale 0.5, align_corners=False) and the two neighbours, in fp32 as PyTorch computes them."""
    f = (np.float32(o) + np.float32(0.5)) * np.float32(0.5) - np.float32(0.5)
    f = np.maximum(f, np.float32(0))
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, (f - i0.astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("TH", [8, 16])
@pytest.mark.parametrize("Hi,Wi", SHAPES)
def test_upfold_indices_weights_and_slots(walker, Hi, Wi, TH):
    out = subprocess.run([walker, str(Hi), str(Wi), str(TH)], check=True, capture_output=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1")).stdout
    t = np.array([[int(v) for v in line.split()] for line in out.decode().splitlines()], dtype=np.int64)
    H, W = 2 * Hi, 2 * Wi
    tiles = -(-H // TH) * -(-W // 32)
    assert t.shape == (tiles * (TH + 2) * 34, 18)                       # every coordinate of every tile, halo included
    ty0, tx0, iy, ix, y0, y1, x0, x1, lyb, lxb, sy0s, sy1s, sx0s, sx1s, cy, cx, sy0, sx0 = t.T
    ush, usw = TH // 2 + 2, 18
    # every coordinate, padding included: indices inside the source, slots inside the scratch
    assert (y0 >= 0).all() and (y1 < Hi).all() and (y0 <= y1).all() and (x0 >= 0).all() and (x1 < Wi).all() and (x0 <= x1).all()
    for s, n in ((sy0s, ush), (sy1s, ush), (sx0s, usw), (sx1s, usw)):
        assert (s >= 0).all() and (s < n).all()
    assert (sy1s - sy0s >= 0).all() and (sy1s - sy0s <= 1).all() and (sx1s - sx0s >= 0).all() and (sx1s - sx0s <= 1).all()
    inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    own = inside & (iy >= ty0) & (iy < ty0 + TH) & (ix >= tx0) & (ix < tx0 + 32)
    assert own.sum() == H * W and len(set(zip(iy[own], ix[own]))) == H * W     # every pixel of the map is some tile's own, once
    # inside the image: PyTorch's indices and weights, as floats; the slot is the source index relative to the tile's origin
    for o, n, i0, i1, lb, s0, s1, org, code in ((iy, Hi, y0, y1, lyb, sy0s, sy1s, sy0, cy), (ix, Wi, x0, x1, lxb, sx0s, sx1s, sx0, cx)):
        w0, w1, wl = torch_axis(o[inside], n)
        assert (i0[inside] == w0).all() and (i1[inside] == w1).all()
        assert (lb[inside].astype(np.uint32) == wl.view(np.uint32)).all()
        assert (s0[inside] == i0[inside] - org[inside]).all() and (s1[inside] == i1[inside] - org[inside]).all()
        assert ((np.float32(0.25) * code[inside].astype(np.float32)).view(np.uint32) == wl.view(np.uint32)).all()   # the packed form
    # the source pixels a slot stands for lie inside the source or are never named by a pixel inside the image
    assert (sy0[inside] + sy0s[inside] >= 0).all() and (sx0[inside] + sx0s[inside] >= 0).all()


def test_conv_up_params_ctypes_layout(tmp_path):
    """sizeof / offsetof of otvm_conv_up_params as the C compiler lays it out == the ctypes mirror, field by field."""
    from otvm_amd import lib as L
    names = [n for n, _ in L.ConvUpParams._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "otvm_hip.h"\nint main(){printf("%zu", sizeof(otvm_conv_up_params));\n'
           + "".join('printf(" %%zu", offsetof(otvm_conv_up_params, %s));\n' % n for n in names) + 'printf("\\n");return 0;}\n')
    exe = str(tmp_path / "up_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(L.ConvUpParams)
    assert got[1:] == [getattr(L.ConvUpParams, n).offset for n in names]
    assert "otvm_conv2d_up" in L.EXPORTED and "otvm_conv2d_accepts_upsampled_input" in L.EXPORTED
