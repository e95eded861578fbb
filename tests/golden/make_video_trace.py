"""Generate tests/golden/video_driver_trace.json.  RUN THIS ON THE PARENT of a commit that restructures otvm_amd/video.py, never on
the commit itself: the fixture pins what run_video_matte and run_video_matte_batch did around the model BEFORE the change -- the
order of frame reads, event waits, backgrounds, conversions, model calls with every keyword, metrics and callbacks, and what was
returned (tests/video_trace.py: a stub model and recorders on the CPU) -- and tests/test_video_driver_cpu.py asserts that the
drivers still do exactly that.

    python -m tests.golden.make_video_trace

To check the committed file, place the parent's otvm_amd/video.py in a copy of the tree and run this there: the result is the
committed file byte for byte.  The fixture holds data only: names, flags, shapes and checksums.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "video_driver_trace.json")


def main():
    from tests import video_trace
    with open(OUT, "w") as f:
        f.write("{")
        for n, name in enumerate(video_trace.CASES):
            with pytest.MonkeyPatch.context() as mp:
                rec = video_trace.record(name, mp)
            f.write('%s\n"%s": {"events": [\n' % ("," if n else "", name))
            f.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in rec["events"]))
            f.write('\n], "returned": %s, "model_after": %s}' % (json.dumps(rec["returned"], separators=(",", ":")),
                                                                  json.dumps(rec["model_after"], separators=(",", ":"))))
            print("%-40s %3d events%s" % (name, len(rec["events"]), "" if rec["returned"] is not None else
                                          "  refused: " + rec["events"][-1][2]))
        f.write("\n}\n")
    print("%s: %d cases, %d bytes" % (OUT, len(video_trace.CASES), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
