"""CPU: what run_video_matte and run_video_matte_batch do around the model -- reads, waits, staging, model calls, metrics, callbacks,
results -- against the trace recorded before the drivers were restructured (tests/video_trace.py, tests/golden/make_video_trace.py).
Exact equality: the fixture is never regenerated from the code under test."""
import json
import os

import pytest

from tests import video_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_driver_trace.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert list(golden) == list(video_trace.CASES)


@pytest.mark.parametrize("name", list(video_trace.CASES))
def test_driver_trace(name, golden, monkeypatch):
    got = json.loads(json.dumps(video_trace.record(name, monkeypatch)))
    want = golden[name]
    for k, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g == w, "event %d of %s" % (k, name)
    assert len(got["events"]) == len(want["events"])
    assert got["returned"] == want["returned"]
    assert got["model_after"] == want["model_after"]
