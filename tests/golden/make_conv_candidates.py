"""Generate tests/golden/conv_candidates.json.  RUN THIS ON THE PARENT of a commit that changes the implicit-GEMM tile table
(otvm_amd/csrc/conv_f16x3_kernel.h: IGEMM_TILES) or the dispatch around it, never on the commit itself: the fixture pins what
otvm_conv2d_candidates offered BEFORE the change, and tests/test_host_logic.py::test_conv_candidates_match_the_recorded_lists
asserts that the library still offers exactly that.

    python -m tests.golden.make_conv_candidates

otvm_conv2d_candidates is host code and the library loads without a GPU; nothing is launched, every pointer is a non-null dummy.
For every layer shape of profiles/r06_autotune_1080p.json and profiles/r06_autotune_480p.json, plus EXTRA below, one list per
combination of: fragment-major weights (w_wfrag) present or not, a split-K workspace or none, precision f16x3 or f16, and -- where
the shape is whole-chunk (Cin % 32 == 0, at most 32 taps) -- a fused input normalisation (in_scale) or none ("cases").

With its compiled-in switches the library offers the LDS-DMA tiles of an f16x3 layer in their 16x16x32 form ONLY (T_M16 + t replaces
T_GLDS + t wherever both are legal, and at f16x3 they are legal together), so no list of "cases" at precision f16x3 holds a
32 + t.  "cases_both_forms" therefore records the f16x3 lists once more from the -DOTVM_PROBES build of the same sources
(libotvm_hip_probes.so beside the library) with OTVM_IGEMM_M16=1, where both forms are offered side by side.  The fixture holds data
only: shapes, flags, lists of integers.
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "conv_candidates.json")
PROFILES = ("r06_autotune_1080p.json", "r06_autotune_480p.json")
DUMMY = 0x10000                   # any non-null, 16-byte aligned address: nothing dereferences it
SPLITK_WS_BYTES = 64 << 20
# shapes the two profiles do not hold, so that every tile is offered in every form it has.  With the default switches the LDS-DMA
# form REPLACES the staged form wherever it is legal; the lists without w_wfrag of the shapes above keep the staged ids, these add
# layers that are not whole-chunk (Cin % 32 != 0: generic decode, staged forms only) at three widths
EXTRA = [
    dict(H=136, W=240, Cin=48, Cout=512, k=3, stride=1, dil=1),
    dict(H=272, W=480, Cin=24, Cout=64, k=1, stride=1, dil=1),
    dict(H=272, W=480, Cin=24, Cout=32, k=3, stride=1, dil=1),
]


def _rup(a, b):
    return (a + b - 1) // b * b


def whole_chunk(shape):
    return _rup(shape["Cin"], 4) % 32 == 0 and shape["k"] * shape["k"] <= 32


def variants(shape):
    """[(w_wfrag, splitk, precision, in_scale)] of a shape, in the fixture's order."""
    return [(wf, sk, prec, ns) for wf in (0, 1) for sk in (0, 1) for prec in (1, 2) for ns in ((0, 1) if whole_chunk(shape) else (0,))]


def key(v):
    return "wfrag%d_splitk%d_prec%d_norm%d" % v


def conv_params(shape, w_wfrag, splitk, precision, in_scale):
    """The otvm_conv_params block of a layer shape as otvm_amd/engine.py (pack_conv_weight, conv_params) fills it, pointers dummy."""
    from otvm_amd import lib as L
    k, stride, dil = shape["k"], shape["stride"], shape["dil"]
    cin = _rup(shape["Cin"], 4)
    cout = shape["Cout"]
    pad = dil * (k - 1) // 2
    p = L.ConvParams()
    p.inp, p.H, p.W, p.Cin, p.in_ld = DUMMY, shape["H"], shape["W"], cin, cin
    p.w, p.K_pad = DUMMY, _rup(k * k * cin, 32)
    p.out, p.Cout, p.out_ld = DUMMY, cout, max(4, _rup(cout, 4))
    p.Ho = (shape["H"] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    p.Wo = (shape["W"] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    p.kh = p.kw = k
    p.stride, p.pad, p.dil = stride, pad, dil
    p.precision = precision
    p.w_hi = p.w_lo = p.w_scale = DUMMY
    if (k == 7 and cout <= 64 and cin <= 64) or (k == 3 and cin % 16 == 0):      # the stem / patch kernel's weight copy
        p.w_frag = DUMMY
    if w_wfrag:
        p.w_wfrag = DUMMY
    if splitk:
        p.splitk_ws, p.splitk_ws_bytes = DUMMY, SPLITK_WS_BYTES
    if in_scale:
        p.in_scale = p.in_shift = DUMMY
    p.batch = 1
    return p


def candidates(lib, p):
    codes = (C.c_int * 128)()
    n = int(lib.otvm_conv2d_candidates(C.byref(p), codes, 128))
    assert 0 <= n < 128
    return [int(codes[i]) for i in range(n)]


def shapes():
    seen, out = set(), []
    for f in PROFILES:
        for e in json.load(open(os.path.join(ROOT, "profiles", f))):
            out.append({k: int(e["shape"][k]) for k in ("H", "W", "Cin", "Cout", "k", "stride", "dil")})
    for s in out + EXTRA:
        t = tuple(sorted(s.items()))
        if t not in seen:
            seen.add(t)
            yield s


def record(lib, precisions=(1, 2)):
    return [{"shape": s, "lists": {key(v): candidates(lib, conv_params(s, *v)) for v in variants(s) if v[2] in precisions}}
            for s in shapes()]


def record_both_forms(lib_path):
    """The f16x3 lists of the probes build beside ``lib_path`` with both LDS-DMA forms offered (a process of its own: the switches
    are read from the environment once, and a process binds one library)."""
    probes = os.path.join(os.path.dirname(lib_path), "libotvm_hip_probes.so")
    assert os.path.exists(probes), "%s is not built (python otvm_amd/csrc/build.py --probes)" % probes
    env = dict(os.environ, OTVM_HIP_LIB=probes, OTVM_IGEMM_M16="1")
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_conv_candidates", "--emit-f16x3"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    from otvm_amd import lib as L
    if "--emit-f16x3" in sys.argv:
        print(json.dumps(record(L.load(), (1,)), separators=(",", ":")))
        return
    parts = {"cases": record(L.load()), "cases_both_forms": record_both_forms(L.LIB_PATH)}
    with open(OUT, "w") as f:
        f.write('{"abi": %d, "splitk_ws_bytes": %d' % (L.ABI_VERSION, SPLITK_WS_BYTES))
        for name, cases in parts.items():
            f.write(',\n"%s": [\n' % name)
            f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))
            f.write("\n]")
        f.write("}\n")
    print("%s: %d shapes, %d lists, %d bytes" % (OUT, len(parts["cases"]), sum(len(c["lists"]) for p in parts.values() for c in p),
                                                 os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
