"""The seven C-ABI handles' refusals on a live handle -- a run before the upload,
a null x / d_x, null results, an upload without the scene or the CartPose
targets the problem needs, a term out of range -- and one good upload and run:
return codes and whole messages equal tests/golden/handle_states.json, recorded
on the commit before the handles moved onto csrc/device_handle.hpp
(tests/golden/make_golden_handle_states.py).  Every refusal returns before a
launch; the good run returns THIP_OK and, where the handle takes a time,
last_ms >= 0."""
import json
from pathlib import Path

import pytest

import handle_states
from trajopt_amd import abi

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "handle_states.json").read_text())


def test_every_handle_is_recorded():
    assert sorted(GOLDEN) == sorted(handle_states.HANDLES)


@pytest.mark.parametrize("handle", sorted(handle_states.HANDLES))
def test_refusals_and_good_run_match_the_recording(handle):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    got = handle_states.HANDLES[handle](abi.load_hip())
    want = GOLDEN[handle]
    for call in want:
        print(handle, call, got.get(call))
    assert list(got) == list(want)  # no call left out, none added
    for call, answer in want.items():
        assert got[call] == answer, (handle, call)
    good = [c for c in got if c.startswith("good_")]
    assert good and all(got[c][0] == 0 for c in good), {c: got[c] for c in good}
    assert got.get("last_ms_ok", True) is True
