"""trajopt::checkTrajectory through the C entry (thost_check_json_batch) without
a GPU: what is refused before any device call, with its reason."""
import json

import numpy as np
import pytest

import dropin_cases as dc
from trajopt_amd import abi, host, problems


@pytest.fixture(scope="module")
def built():
    if not host.HOST_LIB.exists():
        import __graft_entry__

        __graft_entry__.build()
    return host.load_host()


def _problem():
    text = dc.text("arm_around_table.json")
    desc, init, _, _ = host.lower_json(text, dc.arm_around_table_scene())
    return text, desc, init


@pytest.mark.parametrize(
    "cfg, needle",
    [
        (dict(type=5), "type"),
        (dict(type=abi.CHECK_LVS_DISCRETE, lvs=0.0), "lvs"),
        (dict(margin=float("nan")), "margin"),
        (dict(first_step=3, last_step=1), "step range"),
    ],
)
def test_invalid_configs_are_refused_with_their_reason(built, cfg, needle):
    text, desc, init = _problem()
    c = abi.default_check_config()
    for k, v in cfg.items():
        setattr(c, k, v)
    with pytest.raises(host.HostError, match=needle):
        host.check_json_batch([text], dc.arm_around_table_scene()[None], init[None], c)


def test_a_problem_without_a_collision_term_gets_its_environments_model(built):
    """Config B's JSON has no collision term, so its descriptor carries no robot
    spheres; the front door lowers the environment's collision model for the
    check, and what is then refused is the inverted step range, not the model."""
    wl = problems.make_workload("B", 1, n_steps=6)
    text = host.workload_to_json(wl, 0)
    assert "collision" not in {t["type"] for t in json.loads(text)["costs"]}
    desc, init, _, _ = host.lower_json(text)
    assert desc.n_spheres == 0
    c = abi.default_check_config()
    c.first_step, c.last_step = 4, 2
    with pytest.raises(host.HostError, match="step range"):
        host.check_json_batch([text], None, init[None], c)


def test_trajectories_must_match_the_batch(built):
    text, desc, init = _problem()
    with pytest.raises(host.HostError, match="trajectories"):
        host.check_json_batch([text, text], None, init[None])
