"""Solves of the trajopt_sqp front end with the kinematic sets
(thost_tsqp_solve_kin: CartPosConstraint and the fixed-size
DiscreteCollisionConstraint, values and jacobians from the device), with the
reference tests' own solver settings and EXPECTs:
cart_position_optimization_unit.cpp:77-145, numerical_ik_unit.cpp:87-165, a
spherebot collision solve in the spirit of simple_collision_unit.cpp with the
fixed-size set (trajopt_ifopt/test/simple_collision_unit.cpp:115-122), and a
6-node planning-style composition."""
import numpy as np
import pytest

from trajopt_amd import abi, problems, robots, tsqp
from trajopt_amd.runtime import TrajectoryChecker

pytestmark = pytest.mark.gpu

# the tests' OSQP settings: warm start, polish, 8192 iterations, eps_abs 1e-4, eps_rel 1e-6
OSQP = dict(warm_starting=1, polishing=1, max_iter=8192, eps_abs=1e-4, eps_rel=1e-6)
R_TOOL, L_TOOL = "r_gripper_tool_frame", "l_gripper_tool_frame"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    abi.load_hip()
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"


def pose12(T):
    return np.asarray(T)[:3, :].reshape(12)


def quat_wxyz(R):
    """Eigen::Quaterniond(R) (Shoemake's branches)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
    q = np.zeros(4)
    q[0] = (R[k, j] - R[j, k]) / s
    q[1 + i] = 0.25 * s
    q[1 + j] = (R[j, i] + R[i, j]) / s
    q[1 + k] = (R[k, i] + R[i, k]) / s
    return q


def is_approx(a, b, prec):
    """Eigen's isApprox for vectors: |a - b|^2 <= prec^2 min(|a|^2, |b|^2)."""
    return float(((a - b) ** 2).sum()) <= prec * prec * min(float((a ** 2).sum()), float((b ** 2).sum()))


def arm(left):
    chain = robots._chain(robots.PR2_TORSO_WORLD, robots.PR2_LEFT_ARM if left else robots.PR2_RIGHT_ARM)
    lo, hi, _ = robots.chain_limits(chain)
    return chain, lo, hi


def test_cart_position_optimization_unit():
    """right_arm, one node from zero, the tool constrained to the FK of
    (0, 0, 0, -1, 0, -1, 0) in base_footprint; adaptive rho off."""
    chain, lo, hi = arm(False)
    target = robots.fwd_kin(chain, np.array([0.0, 0, 0, -1.0, 0, -1.0, 0]))[robots.PR2_TOOL_LINK]
    spec = tsqp.make_spec(np.zeros((1, 7)), [], var_lower=lo, var_upper=hi, osqp=dict(adaptive_rho=0, **OSQP))
    kin = tsqp.make_kin_spec("right_arm", cart=[dict(node=0, source_frame=R_TOOL, target_frame="base_footprint",
                                                     target_offset=pose12(target))])
    x, r = tsqp.solve_kin(spec, kin)
    got = robots.fwd_kin(chain, x[0])[robots.PR2_TOOL_LINK]
    print(tsqp.STATUS[r.status], r.overall_iteration, x, np.abs(got - target).max())
    assert is_approx(target[:3, 3], got[:3, 3], 1e-4)
    assert is_approx(quat_wxyz(target[:3, :3]), quat_wxyz(got[:3, :3]), 1e-5)
    assert r.qp_setups == 1


def test_numerical_ik_unit():
    """left_arm from (0, 0, 0, -0.001, 0, -0.001, 0) to translation (0.4, 0, 0.8),
    quaternion (w, x, y, z) = (0, 0, 1, 0); adaptive rho on."""
    chain, lo, hi = arm(True)
    target = np.eye(4)
    target[:3, :3] = np.diag([-1.0, 1.0, -1.0])  # Quaterniond(0, 0, 1, 0).toRotationMatrix()
    target[:3, 3] = [0.4, 0.0, 0.8]
    spec = tsqp.make_spec(np.array([[0, 0, 0, -0.001, 0, -0.001, 0]]), [], var_lower=lo, var_upper=hi,
                          osqp=dict(adaptive_rho=1, **OSQP))
    kin = tsqp.make_kin_spec("left_arm", cart=[dict(node=0, source_frame=L_TOOL, target_frame="base_footprint",
                                                    target_offset=pose12(target))])
    x, r = tsqp.solve_kin(spec, kin)
    got = robots.fwd_kin(chain, x[0])[robots.PR2_TOOL_LINK]
    print(tsqp.STATUS[r.status], r.overall_iteration, x, np.abs(got - target).max())
    assert tsqp.STATUS[r.status] == "SQP_CONVERGED"
    assert np.abs(got - target).max() <= 1e-3


def spherebot_check(x):
    """checkTrajectory of spherebot at x [1, 2] against its three static spheres:
    (found, min distance), DISCRETE, contact margin 0 (the reference's manager)."""
    d = abi.ProblemDesc()
    d.n_steps = 1
    d.chain = robots._chain((0.0, 0.0, 0.0), [
        ("spherebot_x_joint", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (1, 0, 0), (-20.0, 20.0)),
        ("spherebot_y_joint", abi.JOINT_PRISMATIC, (0.0, 0.0, 0.0), (0, 1, 0), (-20.0, 20.0)),
        ("spherebot_link_joint", abi.JOINT_FIXED, (0.0, 0.0, 0.0), None, None)])
    d.n_spheres, d.n_prims = 1, 3
    d.sphere_link[0], d.sphere_radius[0] = 3, 0.5
    scene = np.zeros((1, 3, 16))
    for k, c in enumerate([(0.0, 0.0, 0.0), (-0.75, 0.0, 0.0), (0.0, 0.75, 0.0)]):
        scene[0, k, 1:4], scene[0, k, 4] = c, 0.5
    chk = TrajectoryChecker(d, 1, scene, abi.CheckConfig(abi.CHECK_DISCRETE, 1.0, 0.0, 0, -1))
    try:
        res = chk.run(np.asarray(x, dtype=float).reshape(1, 1, 2))[0]
    finally:
        chk.close()
    return bool(res.found), res.min_distance


def test_spherebot_collision_solve():
    """One node starting inside the margin at (-0.75, 0.75): a collision constraint
    (margin 0.2, coeff 1) and a hinge collision cost (margin 0.3, coeff 10), both
    with buffer 0.5 and the fixed-size set (3 rows, fixed sparsity), and the
    JointPos squared cost toward the origin; adaptive rho off."""
    init = np.array([[-0.75, 0.75]])
    terms = [dict(kind=tsqp.JOINT_POS, penalty=tsqp.SQUARED, first=0, coeffs=[1.0, 1.0], lower=[0.0, 0.0])]
    spec = tsqp.make_spec(init, terms, var_lower=[-20.0] * 2, var_upper=[20.0] * 2, osqp=dict(adaptive_rho=0, **OSQP))
    coll = [dict(first=0, margin=0.2, coeff=1.0, buffer=0.5, max_num_cnt=3, fixed_sparsity=True,
                 penalty=tsqp.CONSTRAINT),
            dict(first=0, margin=0.3, coeff=10.0, buffer=0.5, max_num_cnt=3, fixed_sparsity=True, penalty=tsqp.HINGE)]
    x, r = tsqp.solve_kin(spec, tsqp.make_kin_spec("manipulator", coll=coll))
    found0, d0 = spherebot_check(init)
    found1, d1 = spherebot_check(x)
    print(tsqp.STATUS[r.status], r.overall_iteration, r.qp_setups, x, d0, d1)
    assert found0 and d0 < 0
    assert not found1
    assert r.qp_setups == 1  # the resident QP's pattern never changed


def test_six_node_trajectory():
    """The planning-style composition at its smallest: a JointVel squared cost, a
    JointPos constraint on node 0, a CartPos constraint on the last node and
    collision sets as a hinge cost on nodes 1..5, right_arm in config C's scene.
    The scene keeps the reference path 0.075 m clear, so the sets get a margin of
    0.1 (buffer 0.05) to have contacts to work on.  The start trajectory runs
    straight from the workload's first state with the shoulder lift raised by
    0.2 rad, which is clear of the margin (0.104 m by checkTrajectory), to the
    workload's last state (0.080 m clear): the closest state of the start is its
    last node, not node 0, which the JointPos constraint holds only to the
    constraint tolerance -- so the clearance comparison needs no allowance."""
    wl = problems.make_workload("C", 1, n_steps=6)
    chain, lo, hi = arm(False)
    q_start = wl.init[0, 0].copy()
    q_start[1] -= 0.2
    init = np.linspace(q_start, wl.init[0, -1], 6)
    # the goal pose is the FK of a configuration that is itself clear of the margin (0.102 m, the
    # numpy restatement's figure), so it can be reached without going closer than the start
    goal_q = np.clip(init[-1] - 0.1, lo + 0.05, hi - 0.05)
    target = robots.fwd_kin(chain, goal_q)[robots.PR2_TOOL_LINK]
    terms = [dict(kind=tsqp.JOINT_VEL, penalty=tsqp.SQUARED, first=0, last=5, coeffs=[1.0], lower=[0.0] * 7),
             dict(kind=tsqp.JOINT_POS, penalty=tsqp.CONSTRAINT, first=0, coeffs=[1.0] * 7, lower=list(init[0]))]
    spec = tsqp.make_spec(init, terms, var_lower=lo, var_upper=hi, osqp=dict(adaptive_rho=1, **OSQP))
    kin = tsqp.make_kin_spec(
        "right_arm", prims=wl.scene[0],
        cart=[dict(node=5, source_frame=R_TOOL, target_frame="base_footprint", target_offset=pose12(target))],
        coll=[dict(first=1, last=5, margin=0.1, coeff=20.0, buffer=0.05, max_num_cnt=3, fixed_sparsity=True,
                   penalty=tsqp.HINGE)])
    x, r = tsqp.solve_kin(spec, kin)
    got = robots.fwd_kin(chain, x[5])[robots.PR2_TOOL_LINK]
    cfg = abi.CheckConfig(abi.CHECK_DISCRETE, 1.0, 0.0, 0, -1)
    chk = TrajectoryChecker(wl.desc, 1, wl.scene, cfg)

    def moved(traj):  # nodes 1..5 only: node 0 is replaced by node 1 (DISCRETE checks states, not sweeps)
        return np.concatenate([traj[1:2], traj[1:]])[None]

    try:
        s0, s1 = chk.run(init[None])[0], chk.run(x[None])[0]
        c0, c1, t0, t1 = s0.min_distance, s1.min_distance, s0.min_t, s1.min_t
        m0, m1 = chk.run(moved(init))[0].min_distance, chk.run(moved(x))[0].min_distance
    finally:
        chk.close()
    print(tsqp.STATUS[r.status], r.overall_iteration, r.qp_setups, np.abs(got - target).max(), c0, t0, c1, t1, m0, m1)
    assert tsqp.STATUS[r.status] == "SQP_CONVERGED"
    assert np.abs(got - target).max() <= 1e-3
    assert np.abs(x[0] - init[0]).max() <= 1e-4
    # no worse clearance than the start, with no allowance: over the whole trajectory, whose closest
    # state is not the pinned node 0, and over the nodes the solver may move
    assert c0 < 0.1 and t0 != 0
    assert c1 >= c0
    assert m1 >= m0
    assert r.qp_setups == 1
