"""GPU tests of the batch trajopt_sqp front end (thost_tsqp_solve_batch:
trajopt_sqp::BatchTrustRegionSQPSolver over GpuQPBatch and thip_qp_step).  Every
problem of every batch must be, bit for bit, what tsqp.solve / tsqp.solve_kin
gives for it alone: x, status, the iteration counts and the QP counters.  The
solves alone are computed once per problem and shared by the tests."""
import numpy as np
import pytest

import tsqp_cases
from trajopt_amd import abi, problems, robots, tsqp

pytestmark = pytest.mark.gpu

FIELDS = ("status", "overall_iteration", "penalty_iteration", "qp_setups", "qp_updates", "qp_solves", "admm_iters")
_ALONE = {}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"


def alone(kind, seed):
    """(spec, x, Result) of tsqp.solve on its own, computed once."""
    if (kind, seed) not in _ALONE:
        spec = tsqp_cases.synthetic(kind, seed)
        x, r = tsqp.solve(spec)
        x.setflags(write=False)
        _ALONE[(kind, seed)] = (spec, x, r)
    return _ALONE[(kind, seed)]


def check(which, xs, rs):
    """Problem k of the batch against its solve alone."""
    for k, (x1, r1) in enumerate(which):
        got = {f: getattr(rs[k], f) for f in FIELDS}
        want = {f: getattr(r1, f) for f in FIELDS}
        assert got == want, (k, got, want)
        assert xs[k].tobytes() == x1.tobytes(), (k, float(np.abs(xs[k] - x1).max()))


def run(keys):
    ref = [alone(*k) for k in keys]
    xs, rs, rounds, st = tsqp.solve_batch([r[0] for r in ref])
    print(keys, "rounds", st.rounds, "launches", st.step_launches, "groups", st.groups, "max group", st.max_group,
          "qp_rounds", list(rounds))
    check([(r[1], r[2]) for r in ref], xs, rs)
    return rounds, st


@pytest.mark.parametrize("kind", ["smooth", "penalty"])
def test_one_pattern_one_launch_per_round(kind):
    """Four seeds of one kind share the QP pattern: one group, one launch per round.  The problems finish at
    different rounds, and the late ones are what they are alone after the early ones have left."""
    rounds, st = run([(kind, s) for s in range(4)])
    assert st.groups == 1 and st.max_group == 4
    assert st.step_launches == st.rounds == int(rounds.max())
    for k, s in enumerate(range(4)):
        assert rounds[k] >= alone(kind, s)[2].qp_solves  # at least one round per QP solve


def test_two_patterns_two_groups():
    rounds, st = run([("smooth", 0), ("smooth", 1), ("absolute", 0), ("absolute", 1)])
    assert st.groups == 2 and st.max_group == 2
    assert st.rounds == int(rounds.max())
    assert st.rounds <= st.step_launches <= 2 * st.rounds


def test_batch_of_one():
    rounds, st = run([("smooth", 2)])
    assert (st.groups, st.max_group) == (1, 1) and st.step_launches == st.rounds == int(rounds[0])


@pytest.mark.parametrize("kind", ["smooth", "penalty"])
def test_order_independent(kind):
    run([(kind, s) for s in reversed(range(4))])


def test_kinematic_batch():
    """Three right_arm problems of 6 nodes: a CartPos constraint on the last node to three different targets (the FK
    of three seeded joint vectors), a discrete collision hinge cost with fixed sparsity on nodes 1..5, a JointVel cost
    and the pinned first node -- test_gpu_tsqp_kin.py's six-node composition.  Each equals solve_kin alone, and the
    sets' launches are counted."""
    wl = problems.make_workload("C", 1, n_steps=6)
    chain = robots._chain(robots.PR2_TORSO_WORLD, robots.PR2_RIGHT_ARM)
    lo, hi, _ = robots.chain_limits(chain)
    q_start = wl.init[0, 0].copy()
    q_start[1] -= 0.2
    init = np.linspace(q_start, wl.init[0, -1], 6)
    osqp = dict(warm_starting=1, polishing=1, max_iter=8192, eps_abs=1e-4, eps_rel=1e-6, adaptive_rho=1)
    terms = [dict(kind=tsqp.JOINT_VEL, penalty=tsqp.SQUARED, first=0, last=5, coeffs=[1.0], lower=[0.0] * 7),
             dict(kind=tsqp.JOINT_POS, penalty=tsqp.CONSTRAINT, first=0, coeffs=[1.0] * 7, lower=list(init[0]))]
    specs, kins = [], []
    for seed in range(3):
        rng = np.random.default_rng(20261021 + seed)
        goal_q = np.clip(init[-1] - 0.1 + rng.uniform(-0.05, 0.05, 7), lo + 0.05, hi - 0.05)
        target = robots.fwd_kin(chain, goal_q)[robots.PR2_TOOL_LINK]
        specs.append(tsqp.make_spec(init, terms, var_lower=lo, var_upper=hi, osqp=osqp))
        kins.append(tsqp.make_kin_spec(
            "right_arm", prims=wl.scene[0],
            cart=[dict(node=5, source_frame="r_gripper_tool_frame", target_frame="base_footprint",
                       target_offset=np.asarray(target)[:3, :].reshape(12))],
            coll=[dict(first=1, last=5, margin=0.1, coeff=20.0, buffer=0.05, max_num_cnt=3, fixed_sparsity=True,
                       penalty=tsqp.HINGE)]))
    ref = [tsqp.solve_kin(s, k) for s, k in zip(specs, kins)]
    xs, rs, rounds, st = tsqp.solve_batch(specs, kins)
    print("kin rounds", st.rounds, "launches", st.step_launches, "groups", st.groups, "set launches",
          list(st.set_launches), "qp_rounds", list(rounds), [tsqp.STATUS[r.status] for r in rs])
    check(ref, xs, rs)
    assert len({x.tobytes() for x in xs}) == 3  # three different problems
    assert st.rounds == int(rounds.max()) and st.step_launches >= st.rounds
    assert st.set_launches[0] > 0 and st.set_launches[1] > 0
