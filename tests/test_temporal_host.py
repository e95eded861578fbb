"""Host-only side of the temporal stabilisation (no device): the option parsing of otvm_amd/temporal.py and eval_cli, and
run_video_matte's refusals, which come before anything is uploaded."""
import numpy as np
import pytest
import torch

from otvm_amd import temporal
from otvm_amd.eval_cli import parse_stabilise_options
from otvm_amd.video import _Stabilisation, run_video_matte


def test_check_options_takes_the_reciprocals_in_float32():
    k, itc, ita, region = temporal.check_options()
    assert (k, region) == (0.5, "unknown")
    assert itc == float(np.float32(1) / np.float32(24)) and ita == 2.0
    assert temporal.check_options(1, 3.0, 0.1, "all") == (1.0, float(np.float32(1) / np.float32(3)),
                                                          float(np.float32(1) / np.float32(0.1)), "all")
    for kw in (dict(strength=-1e-9), dict(strength=1.0001), dict(strength=float("nan")), dict(strength=True), dict(strength=None),
               dict(tau_colour=0.0), dict(tau_colour=-3), dict(tau_colour=float("inf")), dict(tau_alpha=0), dict(tau_alpha=1e-46),
               dict(tau_alpha=float("nan")), dict(region="band"), dict(region=None)):
        with pytest.raises(ValueError, match="TemporalStabiliser"):
            temporal.check_options(**kw)


def test_options_of():
    assert temporal.options_of(None) is None and temporal.options_of(False) is None
    assert temporal.options_of(True) == {} and temporal.options_of(0) == {"strength": 0.0}
    assert temporal.options_of(0.25) == {"strength": 0.25}
    d = {"strength": 1.0, "tau_colour": 10, "tau_alpha": 0.2, "region": "all"}
    assert temporal.options_of(d) == d and temporal.options_of(d) is not d
    for bad in (1.5, -0.5, "on", [0.5], {"strenght": 0.5}, {"tau_colour": 0}, {"region": "fg"}):
        with pytest.raises(ValueError):
            temporal.options_of(bad)


def test_eval_cli_options():
    assert parse_stabilise_options(None, None, None) is None
    assert parse_stabilise_options(0.5, None, None) == {"strength": 0.5}
    assert parse_stabilise_options(0.8, "12,0.25", "all") == {"strength": 0.8, "tau_colour": 12.0, "tau_alpha": 0.25, "region": "all"}
    for args, why in (((None, "12,0.25", None), "belong to --stabilise"), ((None, None, "all"), "belong to --stabilise"),
                      ((1.5, None, None), "strength"), ((0.5, "12", None), "C,A"), ((0.5, "a,b", None), "C,A"),
                      ((0.5, "1,2,3", None), "C,A"), ((0.5, "0,1", None), "positive"), ((0.5, "5,-1", None), "positive")):
        with pytest.raises(SystemExit, match=why):
            parse_stabilise_options(*args)


class _NoModel:
    """a model nothing may touch: the refusals come before the first look at it beyond its keyframe band"""

    def parameters(self):
        raise AssertionError("the refusal came too late")


def test_run_video_matte_refuses_before_anything_is_uploaded():
    H, W, T = 8, 12, 4
    frames = [np.zeros((H, W, 3), np.uint8) for _ in range(T)]
    tri = np.zeros((3, H, W), np.float32)
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="float"):
        run_video_matte(_NoModel(), [f.astype(np.float32) for f in frames], trimap=tri, stabilise=True, device=dev)
    with pytest.raises(ValueError, match="backgrounds"):
        run_video_matte(_NoModel(), frames, alphas=[np.zeros((H, W), np.float32)] * T, backgrounds=frames, stabilise=0.5, device=dev)
    with pytest.raises(ValueError, match="natural order"):
        run_video_matte(_NoModel(), frames, keyframes={2: tri}, stabilise=True, device=dev)
    with pytest.raises(ValueError, match="natural order"):
        run_video_matte(_NoModel(), frames, keyframes={0: tri, 2: tri}, stabilise=True, device=dev)      # keyframes are issued first
    with pytest.raises(ValueError, match="strength"):
        run_video_matte(_NoModel(), frames, trimap=tri, stabilise=2, device=dev)
    with pytest.raises(ValueError, match="keywords"):
        run_video_matte(_NoModel(), frames, trimap=tri, stabilise={"tau": 1}, device=dev)
    st = _Stabilisation({}, False)
    st.check_frame(torch.zeros((H, W, 3), dtype=torch.uint8))
    for f in (torch.zeros((H, W, 3)), torch.zeros((H, W), dtype=torch.uint8), torch.zeros((H, W, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            st.check_frame(f)
