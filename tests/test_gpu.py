"""GPU parity tests (MI355X): the HIP path through the C-ABI against the oracle.

Bar (BASELINE.json north_star): converged trajectories within 1e-5 absolute
of the CPU path with identical OptStatus and constraint-satisfied flags.  The
gate is tests/parity.py: a problem that misses the bar passes only with a
per-problem proof that the oracle itself does not determine its outcome at
double precision (its reruns under a second rounding of the same algorithm
and under 1e-13 / 1e-12 input perturbations reach the GPU's outcome, or
spread beyond 1e-5).  Batches of 32 or more must meet the bar strictly on
85 % of their problems, and the pooled strict fraction over all checks is
bounded in test_zz_pooled_strict_fraction.
"""
import json
import subprocess
import sys

import numpy as np
import pytest

from parity import RECORDS, TOL_X, check_parity, pooled
from trajopt_amd import abi, problems, robots, sharding
from trajopt_amd.runtime import BatchTrustRegionSQP, HipError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    lib = abi.load_hip()  # raises if the HIP library is missing
    import torch

    assert torch.cuda.is_available(), "gpu tests need an AMD GPU"
    return lib


def solve_gpu(wl, trace=0):
    s = BatchTrustRegionSQP(wl, device=0)
    if trace:
        s.enable_trace(trace)
    x, res = s.optimize()
    tr = s.get_trace() if trace else None
    s.close()
    return x, res, tr


# ------------------------------------------------------------------ kinematics
@pytest.mark.parametrize("robot", ["right_arm", "torso_right_arm", "right_arm_6dof", "right_arm_1dof",
                                   "right_arm_3dof"])
def test_fwd_kin_parity(oracle_mod, robot):
    wl = problems.make_workload("B", 4, robot=robot)
    s = BatchTrustRegionSQP(wl)
    poses = s.fwd_kin(wl.init)
    s.close()
    ref = oracle_mod.fwd_kin(wl.desc.chain, wl.init.reshape(-1, wl.n_dof)).reshape(poses.shape)
    np.testing.assert_allclose(poses, ref, rtol=0, atol=1e-13)


def test_fwd_kin_parity_dual_arm_tree(oracle_mod):
    """Config E's 14-DoF both_arms group (two branches off torso_lift_link):
    every link's pose on the GPU against the oracle and the numpy FK."""
    wl = problems.make_workload("E", 4, n_steps=6)
    s = BatchTrustRegionSQP(wl)
    poses = s.fwd_kin(wl.init)
    s.close()
    q = wl.init.reshape(-1, wl.n_dof)
    ref = oracle_mod.fwd_kin(wl.desc.chain, q).reshape(poses.shape)
    np.testing.assert_allclose(poses, ref, rtol=0, atol=1e-13)
    T = robots.fwd_kin(wl.desc.chain, q[7])
    for k in range(wl.desc.chain.n_links):
        np.testing.assert_allclose(poses.reshape(-1, wl.desc.chain.n_links, 12)[7, k],
                                   T[k][:3, :].reshape(12), rtol=0, atol=1e-12)


def test_fwd_kin_golden(golden):
    g = golden("fk_pr2")
    wl = problems.make_workload("A", 16, n_steps=2)
    q = np.repeat(g["q"][:, None, :], 2, axis=1)
    s = BatchTrustRegionSQP(wl)
    poses = s.fwd_kin(q)
    s.close()
    np.testing.assert_allclose(poses[:, 0], g["poses"], rtol=0, atol=1e-13)


@pytest.mark.parametrize("cfg,B", [("A", 8), ("B", 8)])
def test_cartpose_linearization_parity(oracle_mod, cfg, B):
    wl = problems.make_workload(cfg, B)
    rng = np.random.default_rng(7)
    x = wl.init + rng.normal(0, 0.05, wl.init.shape)
    s = BatchTrustRegionSQP(wl)
    err, jac = s.linearize(x)
    s.close()
    eo, jo = oracle_mod.linearize(wl, x)
    np.testing.assert_allclose(err, eo, rtol=0, atol=1e-12)
    # forward differences with eps = 1e-5 (kinematic_terms.hpp:15) amplify
    # last-bit FK differences by 1e5
    np.testing.assert_allclose(jac, jo, rtol=0, atol=1e-9)


@pytest.mark.parametrize("robot", ["right_arm_1dof", "right_arm_3dof"])
def test_cartpose_linearization_parity_small_chains(oracle_mod, robot):
    """test_cartpose_linearization_parity's check on config B over chains of 1 and 3 dofs
    (robots.ROBOTS: the later joints held fixed): Jacobians of 1 and 3 columns."""
    wl = problems.make_workload("B", 8, robot=robot)
    rng = np.random.default_rng(7)
    x = wl.init + rng.normal(0, 0.05, wl.init.shape)
    s = BatchTrustRegionSQP(wl)
    err, jac = s.linearize(x)
    s.close()
    eo, jo = oracle_mod.linearize(wl, x)
    assert jac.shape[-1] == wl.n_dof == int(robot[-4]) and np.abs(jo).max() > 0.1
    np.testing.assert_allclose(err, eo, rtol=0, atol=1e-12)
    np.testing.assert_allclose(jac, jo, rtol=0, atol=1e-9)


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_cartpose_linearization_parity_tolerance(oracle_mod, cfg):
    """Toleranced CartPose rows (applyTolerances on the error, the tolerance-aware
    error difference in the FD jacobian): some components inside their band (zero
    rows), some outside."""
    wl = problems.with_cart_tolerances(problems.make_workload(cfg, 16), pos=0.02, rot=0.1)
    rng = np.random.default_rng(11)
    x = wl.init + rng.normal(0, 0.05, wl.init.shape)
    s = BatchTrustRegionSQP(wl)
    err, jac = s.linearize(x)
    s.close()
    eo, jo = oracle_mod.linearize(wl, x)
    assert (eo == 0).any() and (eo != 0).any()
    np.testing.assert_allclose(err, eo, rtol=0, atol=1e-12)
    np.testing.assert_allclose(jac, jo, rtol=0, atol=1e-9)


def test_cartpose_linearization_parity_dynamic(oracle_mod):
    """DynamicCartPose rows (both frames active, kinematic_terms.cpp:58-187): the
    target is an arm link, the FD jacobian perturbs both frames."""
    wl = problems.with_dynamic_target(problems.make_workload("B", 16))
    rng = np.random.default_rng(13)
    x = wl.init + rng.normal(0, 0.05, wl.init.shape)
    s = BatchTrustRegionSQP(wl)
    err, jac = s.linearize(x)
    s.close()
    eo, jo = oracle_mod.linearize(wl, x)
    assert np.abs(eo).max() > 1e-3
    # columns of joints upstream of the target link move both frames alike: zero there
    assert np.abs(jo[..., :2]).max() < 1e-6
    np.testing.assert_allclose(err, eo, rtol=0, atol=1e-12)
    np.testing.assert_allclose(jac, jo, rtol=0, atol=1e-9)


def test_cartpose_linearization_golden_tolerance(golden):
    g = golden("cartpose_B_tol")
    wl = problems.with_cart_tolerances(problems.make_workload("B", g["x"].shape[0]))
    s = BatchTrustRegionSQP(wl)
    err, jac = s.linearize(g["x"])
    s.close()
    np.testing.assert_allclose(err, g["err"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(jac, g["jac"], rtol=0, atol=1e-9)


def test_cartpose_inverted_tolerance_band_rejected():
    wl = problems.with_cart_tolerances(problems.make_workload("A", 2))
    wl.desc.cart_lower_tol[0][3] = 0.3
    with pytest.raises(HipError, match="Inverted tolerance band"):
        BatchTrustRegionSQP(wl)


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_cartpose_linearization_golden(golden, cfg):
    g = golden(f"cartpose_{cfg}")
    wl = problems.make_workload(cfg, g["x"].shape[0])
    s = BatchTrustRegionSQP(wl)
    err, jac = s.linearize(g["x"])
    s.close()
    np.testing.assert_allclose(err, g["err"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(jac, g["jac"], rtol=0, atol=1e-9)


# ------------------------------------------------------------------ SQP parity
def _jv(batch, n_steps=12):
    wl = problems.make_workload("B", batch, n_steps=n_steps)
    wl.desc.n_cart = 0
    wl.targets = np.zeros((batch, 0, 12))
    return wl


def test_sqp_golden_fixtures(golden, oracle_mod):
    for name, wl in (("sqp_A", problems.make_workload("A", 8)), ("sqp_B", problems.make_workload("B", 2)),
                     ("sqp_jv", _jv(4))):
        g = golden(name)
        x, res, _ = solve_gpu(wl)
        np.testing.assert_array_equal([r.status for r in res], g["status"], err_msg=name)
        close = np.abs(x - g["x"]).reshape(wl.batch, -1).max(1) <= TOL_X
        if not close.all():
            check_parity(wl, oracle_mod, x, res, label=name)


@pytest.mark.parametrize("cfg,B", [("A", 64), ("B", 32)])
def test_sqp_parity(oracle_mod, cfg, B):
    wl = problems.make_workload(cfg, B)
    x, res, _ = solve_gpu(wl)
    check_parity(wl, oracle_mod, x, res, label=cfg)


def _first_qp_l1(wl, b_list, gpu_trace, oracle_mod):
    """sum |x*| of the first QP of each listed problem: (GPU trace, oracle trace)."""
    out = []
    for b in b_list:
        _, _, to = oracle_mod.solve_trace(wl, b, cap=4096)
        out.append((gpu_trace[b][0][8], to[0][8]))
    return np.array(out)


def test_jitter_amplitudes_match_measured_gaps(oracle_mod):
    """The parity gate's rounding jitter (parity.JITTER) against the measured
    GPU-vs-oracle gap of the same quantity on the fused path:
      * forward-difference CartPose Jacobian entries (thip_linearize vs the
        oracle at config C's initial trajectories, 64 problems), absolute;
      * one KKT solve: config J (JointPos terms only, so the first QP's data
        are exact on both sides) with one ADMM iteration per QP (max_iter 1,
        no adaptive rho, no polish): the first QP's iterate is one scaled KKT
        solve -- the twisted block factor against the oracle's LDL^T --
        compared as sum |x| (trace records), relative;
      * QP solutions: the first QP's step (the trajectory after one SQP
        iteration minus the start), element-wise relative to the step, config
        J and config C (whose data carry the Jacobian gap);
      * contact expressions (collision gradient coefficients and constant):
        thip_collision_rows against the oracle's rows on config C, LVS_DISCRETE
        and LVS_CONTINUOUS, at the initial and solved trajectories, absolute.
    Each amplitude covers the largest measured gap of its quantity and lies
    within 30x of it: the jitter re-draws the GPU's rounding without swamping
    it."""
    from parity import JITTER

    wl = problems.make_workload("C", 64)
    s = BatchTrustRegionSQP(wl)
    _, Jg = s.linearize(wl.init)
    s.close()
    _, Jo = oracle_mod.linearize(wl, wl.init)
    gap_jac = float(np.abs(Jg - Jo).max())
    B = 16
    rel = lambda v: float(np.max(np.abs(v[:, 0] - v[:, 1]) / np.abs(v[:, 1])))  # noqa: E731
    wl1 = problems.make_workload("J", B)
    wl1.desc.osqp.max_iter, wl1.desc.osqp.check_termination = 1, 0
    wl1.desc.osqp.adaptive_rho, wl1.desc.osqp.polishing = 0, 0
    wl1.desc.sqp.max_iter = 1
    _, _, tr = solve_gpu(wl1, trace=64)
    gap_kkt = rel(_first_qp_l1(wl1, range(B), tr, oracle_mod))
    # QP solutions element-wise: the trajectory after one SQP iteration is x0 plus the
    # first QP's step (config J: exact data; config C: the data carry the Jacobian gap)
    def first_step_gap(wls):
        wls.desc.sqp.max_iter = 1
        xg, _, _ = solve_gpu(wls)
        xo, _ = oracle_mod.solve(wls, n_threads=16)
        step = np.abs(xo - wls.init).reshape(B, -1).max(1)
        return float(np.max(np.abs(xg - xo).reshape(B, -1).max(1) / np.maximum(step, 1e-300)))

    gap_sol = first_step_gap(problems.make_workload("J", B))
    gap_sol_c = first_step_gap(problems.make_workload("C", B))
    # contact expressions: the fused kernel's rows against the oracle's, config C (LVS_DISCRETE and
    # LVS_CONTINUOUS) at the initial and the oracle-solved trajectories
    gap_coll = 0.0
    for cont in (0, 1):
        wlr = problems.make_workload("C", 16, first_problem=200)
        wlr.desc.coll_continuous = cont
        xo, _ = oracle_mod.solve(wlr, n_threads=16)
        s = BatchTrustRegionSQP(wlr)
        for xx in (wlr.init, xo):
            rows = s.collision_rows(xx)
            for b in range(wlr.batch):
                rc = oracle_mod.collision_rows(wlr, b, xx[b])
                assert rows[b].shape == rc.shape
                if len(rc):
                    gap_coll = max(gap_coll, float(np.abs(rows[b][:, 8:] - rc[:, 8:]).max()))
        s.close()
    print(f"measured gaps: FD jacobian {gap_jac:.2e} (jitter {JITTER[0]:.0e}); one KKT solve {gap_kkt:.2e} "
          f"(jitter {JITTER[1]:.0e}); QP solution J {gap_sol:.2e}, C {gap_sol_c:.2e} (jitter {JITTER[2]:.0e}); "
          f"contact expressions {gap_coll:.2e} (jitter {JITTER[3]:.0e})")
    for name, gap, amp in (("FD jacobian", gap_jac, JITTER[0]), ("KKT solve", gap_kkt, JITTER[1]),
                           ("QP solution", max(gap_sol, gap_sol_c), JITTER[2]),
                           ("contact expressions", gap_coll, JITTER[3])):
        # (a gap below one ulp counts as one ulp: the floor of any rounding difference)
        assert gap <= amp <= 30 * max(gap, 2.2e-16), f"{name}: jitter {amp:.1e} vs measured gap {gap:.2e}"


# ------------------------------------------------------------------ collision (config C)
def _check_rows(rg, rc, label, cc_atol=0.0):
    assert rg.shape == rc.shape, f"{label}: {len(rg)} contact rows vs {len(rc)}"
    if len(rc) == 0:
        return
    # identity and order: step pair, link, primitive, sphere, sub-state, kept coefficients
    np.testing.assert_array_equal(rg[:, [0, 1, 2, 3, 4, 7]], rc[:, [0, 1, 2, 3, 4, 7]], err_msg=label)
    np.testing.assert_allclose(rg[:, 5], rc[:, 5], rtol=0, atol=1e-12, err_msg=label)   # distance
    # cc_time: exact for sub-states; a cast's closest-point time is a closed-form
    # quotient, equal to rounding (the GPU contracts multiply-adds)
    np.testing.assert_allclose(rg[:, 6], rc[:, 6], rtol=0, atol=cc_atol, err_msg=label)
    np.testing.assert_allclose(rg[:, 8:], rc[:, 8:], rtol=0, atol=1e-11, err_msg=label)  # gradient row, constant


def test_collision_rows_parity(oracle_mod):
    wl = problems.make_workload("C", 16)
    xo, _ = oracle_mod.solve(wl, n_threads=16)
    s = BatchTrustRegionSQP(wl)
    rows = s.collision_rows(xo)
    rows_init = s.collision_rows(wl.init)
    s.close()
    assert sum(len(r) for r in rows) > 100
    for b in range(wl.batch):
        _check_rows(rows[b], oracle_mod.collision_rows(wl, b, xo[b]), f"problem {b} (solution)")
        _check_rows(rows_init[b], oracle_mod.collision_rows(wl, b, wl.init[b]), f"problem {b} (init)")


@pytest.mark.parametrize("robot", ["right_arm_1dof", "right_arm_3dof"])
def test_collision_rows_parity_small_chains(oracle_mod, robot):
    """Config C's contact rows over chains of 1 and 3 dofs (robots.ROBOTS: the later joints
    held fixed, so the spheres of the held links still collide but their gradient rows have
    1 or 3 columns per waypoint), at the initial and at a perturbed trajectory.  A contact
    distance of 0.325 m (coll_buffer 0.3) gives every problem thousands of rows."""
    wl = problems.make_workload("C", 4, robot=robot)
    wl.desc.coll_buffer = 0.3
    x = wl.init + np.random.default_rng(7).normal(0, 0.05, wl.init.shape)
    s = BatchTrustRegionSQP(wl)
    rows_init = s.collision_rows(wl.init, cap=8192)
    rows = s.collision_rows(x, cap=8192)
    s.close()
    assert min(len(r) for r in rows_init) > 1000 and rows[0].shape[1] == 8 + 2 * int(robot[-4]) + 1
    for b in range(wl.batch):
        _check_rows(rows_init[b], oracle_mod.collision_rows(wl, b, wl.init[b]), f"problem {b} (init)")
        _check_rows(rows[b], oracle_mod.collision_rows(wl, b, x[b]), f"problem {b} (perturbed)")


def _continuous(wl):
    wl.desc.coll_continuous = 1  # LVS_CONTINUOUS: swept spheres between sub-states
    return wl


def test_collision_rows_parity_continuous(oracle_mod):
    """LVS_CONTINUOUS (CastCollisionEvaluator, collision_terms.cpp:978-1161)
    contacts and distance expressions against the oracle at the initial and
    the solved trajectories."""
    wl = _continuous(problems.make_workload("C", 16))
    xo, _ = oracle_mod.solve(wl, n_threads=16)
    s = BatchTrustRegionSQP(wl)
    rows = s.collision_rows(xo)
    rows_init = s.collision_rows(wl.init)
    s.close()
    assert sum(len(r) for r in rows_init) > 40
    for b in range(wl.batch):
        _check_rows(rows[b], oracle_mod.collision_rows(wl, b, xo[b]), f"problem {b} (solution)", cc_atol=1e-12)
        _check_rows(rows_init[b], oracle_mod.collision_rows(wl, b, wl.init[b]), f"problem {b} (init)", cc_atol=1e-12)


def test_collision_rows_parity_dual_arm(oracle_mod):
    """Config E: LVS_CONTINUOUS contacts of both arms' spheres (links on two
    branches of the tree; gradients through each arm's own joints) against
    the oracle at the initial trajectory."""
    wl = problems.make_workload("E", 8, n_steps=12)
    wl.desc.coll_buffer = 0.3  # contacts within 0.325 m: every problem has some
    s = BatchTrustRegionSQP(wl)
    rows_init = s.collision_rows(wl.init)
    s.close()
    assert all(len(r) > 0 for r in rows_init)
    for b in range(wl.batch):
        _check_rows(rows_init[b], oracle_mod.collision_rows(wl, b, wl.init[b]), f"problem {b} (init)", cc_atol=1e-12)


def test_collision_rows_parity_self(oracle_mod):
    """Robot self-collision (the link pairs pr2.srdf's ACM leaves enabled): on a
    crossed-arms trajectory of config E the fused kernel's contact rows -- the
    scene keys, then the self keys, both links' gradients -- match the oracle,
    for LVS_CONTINUOUS (each side its own closest-point time along its cast)
    and LVS_DISCRETE; the device evaluator of the generic path gives the same
    records."""
    from test_collision import _dual_arm_crossing
    from trajopt_amd.runtime import TermEvaluator
    wl = problems.make_workload("E", 4, n_steps=12)
    rng = np.random.default_rng(11)
    q = [_dual_arm_crossing(wl, rng) for _ in range(wl.batch)]
    # a trajectory sweeping through the crossing: casts with distinct end states
    x = np.stack([qb[None, :] + 0.02 * np.sin(np.arange(wl.n_steps)[:, None] + np.arange(wl.n_dof)[None, :])
                  for qb in q])
    for cont in (1, 0):
        wl.desc.coll_continuous = cont
        s = BatchTrustRegionSQP(wl)
        rows = s.collision_rows(x)
        s.close()
        n_self = 0
        for b in range(wl.batch):
            rc = oracle_mod.collision_rows(wl, b, x[b])
            _check_rows(rows[b], rc, f"problem {b} (continuous {cont})", cc_atol=1e-12)
            n_self += int((rc[:, 2] < 0).sum())
        assert n_self > 0
        ev = TermEvaluator(wl)
        try:
            recs = ev.collision(0, x)
        finally:
            ev.close()
        for b in range(wl.batch):
            _check_rows(recs[b], oracle_mod.collision_rows(wl, b, x[b]), f"eval problem {b} (continuous {cont})",
                        cc_atol=1e-12)


def test_sqp_parity_dual_arm_E(oracle_mod):
    """Config E (BASELINE.json configs[4]): 14-DoF dual arm, 50 waypoints,
    both tool frames tracked, LVS_CONTINUOUS collision including the inter-arm
    self-collision pairs -- they couple the arms, so the block solve runs the
    14-dof wide path."""
    wl = problems.make_workload("E", 4)
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    xo, ro = oracle_mod.solve(wl, n_threads=16)
    # strict on these four: same status, x within the bar, the same SQP path
    for b in range(wl.batch):
        assert res[b].status == ro[b].status, b
        assert np.abs(x[b] - xo[b]).max() <= TOL_X, (b, np.abs(x[b] - xo[b]).max())
        assert (res[b].n_sqp_iters, res[b].n_qp_solves) == (ro[b].n_sqp_iters, ro[b].n_qp_solves), b
    check_parity(wl, oracle_mod, x, res, label="E", oracle=(xo, ro))


def test_sqp_parity_collision_continuous(oracle_mod):
    wl = _continuous(problems.make_workload("C", 32, first_problem=200))
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    check_parity(wl, oracle_mod, x, res, label="C-continuous")
    wl = _continuous(problems.make_workload("C", 8, first_problem=300))
    wl.desc.coll_is_cnt = 1
    x, res, _ = solve_gpu(wl)
    check_parity(wl, oracle_mod, x, res, label="C-continuous-cnt")


def _single(wl):
    wl.desc.coll_continuous = 2  # DISCRETE: SingleTimestepCollisionEvaluator per free waypoint
    wl.desc.coll_buffer = 0.1  # (at the waypoints alone the 0.05 buffer finds few contacts)
    return wl


def test_collision_rows_parity_discrete(oracle_mod):
    """DISCRETE (SingleTimestepCollisionEvaluator, collision_terms.cpp:538-554,
    600-688): one term per free waypoint, contacts at q_t, gradient scale 1."""
    wl = _single(problems.make_workload("C", 16))
    wl.desc.coll_n_fixed = 2
    wl.desc.coll_fixed_steps[1] = 7  # a fixed interior waypoint has no term
    xo, _ = oracle_mod.solve(wl, n_threads=16)
    s = BatchTrustRegionSQP(wl)
    rows = s.collision_rows(xo)
    rows_init = s.collision_rows(wl.init)
    s.close()
    assert sum(len(r) for r in rows_init) > 40
    for b in range(wl.batch):
        for r in (rows[b], rows_init[b]):
            assert not np.isin(r[:, 0], [0, 7]).any()
        _check_rows(rows[b], oracle_mod.collision_rows(wl, b, xo[b]), f"problem {b} (solution)")
        _check_rows(rows_init[b], oracle_mod.collision_rows(wl, b, wl.init[b]), f"problem {b} (init)")


def test_sqp_parity_collision_discrete(oracle_mod):
    wl = _single(problems.make_workload("C", 32, first_problem=400))
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    assert all(r.n_costs == 1 + 29 + (wl.n_steps - 1) for r in res)
    check_parity(wl, oracle_mod, x, res, label="C-discrete")
    wl = _single(problems.make_workload("C", 8, first_problem=500))
    wl.desc.coll_is_cnt = 1
    x, res, _ = solve_gpu(wl)
    assert all(r.n_cnts == wl.n_steps - 1 for r in res)
    check_parity(wl, oracle_mod, x, res, label="C-discrete-cnt")


def test_collision_rows_golden_discrete(golden):
    g = golden("collision_rows_C_single")
    wl = _single(problems.make_workload("C", 3))
    s = BatchTrustRegionSQP(wl)
    rows = s.collision_rows(g["x"])
    s.close()
    for b in range(3):
        _check_rows(rows[b], g[f"rows{b}"], f"golden discrete problem {b}")


def test_collision_rows_golden(golden):
    g = golden("collision_rows_C")
    wl = problems.make_workload("C", 3)
    s = BatchTrustRegionSQP(wl)
    rows = s.collision_rows(g["x"])
    s.close()
    for b in range(3):
        _check_rows(rows[b], g[f"rows{b}"], f"golden problem {b}")


def test_collision_rows_golden_continuous(golden):
    g = golden("collision_rows_C_cont")
    wl = _continuous(problems.make_workload("C", 3))
    s = BatchTrustRegionSQP(wl)
    rows = s.collision_rows(g["x"])
    s.close()
    for b in range(3):
        _check_rows(rows[b], g[f"rows{b}"], f"golden continuous problem {b}", cc_atol=1e-12)


def test_sqp_parity_collision(oracle_mod, golden):
    g = golden("sqp_C")
    wl = problems.make_workload("C", 3)
    x, res, _ = solve_gpu(wl)
    np.testing.assert_array_equal([r.status for r in res], g["status"])
    assert np.abs(x - g["x"]).max() <= TOL_X
    wl = problems.make_workload("C", 32)
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    check_parity(wl, oracle_mod, x, res, label="C")


def test_sqp_parity_collision_constraint(oracle_mod):
    """CollisionConstraint (LVS-discrete, collision_terms.cpp:1308-1386) as a
    constraint: ineq rows coeff*(margin - dist) inflated by the per-step-pair
    merit coefficients, violations counted in the penalty loop."""
    wl = problems.make_workload("C", 16, first_problem=64)
    wl.desc.coll_is_cnt = 1
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    assert all(r.n_cnts == wl.n_steps - 1 for r in res)
    check_parity(wl, oracle_mod, x, res, label="C-cnt")


def test_collision_rows_parity_pairs(oracle_mod):
    """Per link-pair margins and coefficients (CollisionTermInfo "pairs",
    problem_description.cpp:1686-1719; thip_coll_pair): the fused kernel's and
    the device evaluator's contact rows -- each pair's own contact distance, a
    zero-coefficient pair dropped, a self pair with its own margin -- against the
    oracle at the initial and the solved trajectories."""
    from trajopt_amd.runtime import TermEvaluator

    wl = problems.with_pair_data(problems.make_workload("C", 16))
    # five scene pair entries (one replaced), plus a self pair when the arm has self-collision pairs
    assert wl.desc.n_coll_pairs == 5 + (1 if wl.desc.n_self_pairs > 0 else 0)
    xo, _ = oracle_mod.solve(wl, n_threads=16)
    s = BatchTrustRegionSQP(wl)
    rows = {"init": s.collision_rows(wl.init), "solution": s.collision_rows(xo)}
    s.close()
    ev = TermEvaluator(wl)
    try:
        recs = {"init": ev.collision(0, wl.init), "solution": ev.collision(0, xo)}
    finally:
        ev.close()
    n = 0
    for tag, x in (("init", wl.init), ("solution", xo)):
        for b in range(wl.batch):
            rc = oracle_mod.collision_rows(wl, b, x[b])
            _check_rows(rows[tag][b], rc, f"problem {b} ({tag})")
            _check_rows(recs[tag][b], rc, f"eval problem {b} ({tag})")
            n += len(rc)
    assert n > 100


def test_sqp_parity_collision_pairs(oracle_mod):
    """SQP parity with per link-pair data on the collision cost (hinge rows with
    their pair's margin in the bound and coefficient in the objective) and on
    the collision constraint (the pair's coefficient scales its row,
    exprMult(margin - dist, coeff), collision_terms.cpp:1347-1386)."""
    wl = problems.with_pair_data(problems.make_workload("C", 32, first_problem=96))
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    check_parity(wl, oracle_mod, x, res, label="C-pairs")
    wl = problems.with_pair_data(problems.make_workload("C", 16, first_problem=160))
    wl.desc.coll_is_cnt = 1
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    check_parity(wl, oracle_mod, x, res, label="C-cnt-pairs")


def test_frontdoor_json_pairs_parity(oracle_mod):
    """JSON problems whose collision term carries "pairs" (robot link against a
    scene object named scene_<p>, a zero coefficient, a self pair) through the
    C++ front door onto the fused kernel, against the oracle on the lowered
    problems; and the same problems with a second collision term (the generic
    host loop: device-evaluated collision terms with per-record pair data)."""
    import json as _json

    from trajopt_amd import host

    wl0 = problems.make_workload("C", 4)
    texts = []
    for b in range(4):
        doc = _json.loads(host.workload_to_json(wl0, b))
        for t in doc["costs"]:
            if t["type"] == "collision":
                t["params"]["pairs"] = [
                    {"link": "r_wrist_roll_link", "pair": ["scene_1", "scene_2"], "coeffs": 40, "dist_pen": 0.04},
                    {"link": "scene_0", "pair": ["r_forearm_roll_link"], "coeffs": 0, "dist_pen": 0.02},
                    {"link": "r_shoulder_pan_link", "pair": ["r_wrist_flex_link"], "coeffs": 5, "dist_pen": 0.03}]
        texts.append(_json.dumps(doc))
    scenes = np.ascontiguousarray(wl0.scene[:, :3])
    x, res = host.solve_json_batch(texts, scenes)
    wl = _lowered_workload(texts, scenes)
    assert wl.desc.n_coll_pairs == 4
    check_parity(wl, oracle_mod, x, res, label="json-pairs")
    # a second collision term (a constraint with pairs of its own): the host loop
    # (one problem on a 5-waypoint horizon: the generic path's sparse-LDL QPs on
    # a 30-waypoint collision problem take minutes)
    wls = problems.make_workload("C", 1, n_steps=5)
    doc = _json.loads(host.workload_to_json(wls, 0))
    for t in doc["costs"]:
        if t["type"] == "collision":
            t["params"]["pairs"] = [
                {"link": "r_wrist_roll_link", "pair": ["scene_1", "scene_2"], "coeffs": 40, "dist_pen": 0.04},
                {"link": "scene_0", "pair": ["r_forearm_roll_link"], "coeffs": 0, "dist_pen": 0.02},
                {"link": "r_shoulder_pan_link", "pair": ["r_wrist_flex_link"], "coeffs": 5, "dist_pen": 0.03}]
    doc["constraints"].append({"type": "collision", "params": {
        "coeffs": 10, "dist_pen": 0.01, "evaluator_type": 2,
        "pairs": [{"link": "r_wrist_roll_link", "pair": ["scene_1"], "coeffs": 3, "dist_pen": 0.0}]}})
    texts2 = [_json.dumps(doc)]
    scenes2 = np.ascontiguousarray(wls.scene[:, :3])
    x2, res2 = host.solve_json_batch(texts2, scenes2)
    wl2 = _lowered_workload(texts2, scenes2)
    assert wl2.desc.n_coll_extra == 1 and wl2.desc.n_coll_pairs == 5
    assert host.last_batch_qp_stats()[1] > 0  # the host loops ran
    check_parity(wl2, oracle_mod, x2, res2, label="json-pairs-generic")


def _variant(name):
    if name == "jointvel_only":
        return _jv(6)
    if name == "short_horizon":
        return problems.make_workload("A", 8, n_steps=5)
    if name == "two_fixed_steps":
        wl = problems.make_workload("A", 8)
        wl.desc.n_fixed = 2
        wl.desc.fixed_steps[1] = 1
        return wl
    if name == "position_only_cartpose":
        wl = problems.make_workload("A", 8)
        for i in range(3):
            wl.desc.cart_rot_coeffs[0][i] = 0.0
        return wl
    if name == "admm_iteration_cap":
        wl = problems.make_workload("A", 8)
        wl.desc.osqp.max_iter = 60
        return wl
    if name == "sqp_iteration_cap":
        wl = problems.make_workload("A", 8)
        wl.desc.sqp.max_iter = 3
        return wl
    if name == "sqp_iteration_cap_costs_only":
        wl = problems.make_workload("B", 4)
        wl.desc.sqp.max_iter = 3
        return wl
    if name == "no_scaling":
        wl = problems.make_workload("A", 8)
        wl.desc.osqp.scaling = 0
        return wl
    if name == "no_polish":
        wl = problems.make_workload("A", 8)
        wl.desc.osqp.polishing = 0
        return wl
    if name == "no_adaptive_rho_no_warm_start":
        wl = problems.make_workload("A", 8)
        wl.desc.osqp.adaptive_rho = 0
        wl.desc.osqp.warm_starting = 0
        return wl
    if name == "jointpos_goal":
        return problems.make_workload("J", 32)
    if name == "jointpos_goal_offset":
        return problems.make_workload("J", 16, goal_offset=0.05, first_problem=100)
    if name == "jointpos_far_goal_penalty_limit":
        return problems.make_workload("J", 8, goal_offset=0.3)
    if name == "jointpos_with_cartpose":
        wl = problems.make_workload("A", 8)
        d = wl.desc
        d.n_jpos = 1
        d.jpos_is_cnt[0] = 0
        d.jpos_first_step[0] = 2
        d.jpos_last_step[0] = -1
        for j in range(wl.n_dof):
            d.jpos_coeffs[0][j] = 0.5
            d.jpos_targets[0][j] = float(wl.q_ref[0, 4, j])
        return wl
    if name == "jointvel_ineq_cost":
        # JointVelIneqCost (trajectory_costs.cpp:303-374): velocity band instead of the quadratic
        wl = problems.make_workload("J", 16)
        for j in range(wl.n_dof):
            wl.desc.jv_upper_tols[j] = 0.05
            wl.desc.jv_lower_tols[j] = -0.05
        return wl
    if name == "jointpos_ineq_cost_and_cnt":
        wl = problems.make_workload("A", 8)
        d = wl.desc
        d.n_jpos = 2
        mid = wl.q_ref[0, 4]
        for k, (cnt, first, last, c, tol) in enumerate([(1, 4, 4, 1.0, 0.3), (0, 1, -1, 2.0, 0.05)]):
            d.jpos_is_cnt[k], d.jpos_first_step[k], d.jpos_last_step[k] = cnt, first, last
            for j in range(wl.n_dof):
                d.jpos_coeffs[k][j] = c
                d.jpos_targets[k][j] = float(mid[j])
                d.jpos_upper_tols[k][j] = tol
                d.jpos_lower_tols[k][j] = -tol
        return wl
    if name == "collision_with_static_hinges":
        # contacts and JointPos hinge rows share the step pairs (contacts first)
        wl = problems.make_workload("C", 8)
        d = wl.desc
        d.n_jpos = 1
        d.jpos_is_cnt[0], d.jpos_first_step[0], d.jpos_last_step[0] = 0, 0, -1
        lo, hi, _ = robots.chain_limits(d.chain)
        for j in range(wl.n_dof):
            d.jpos_coeffs[0][j] = 0.5
            d.jpos_targets[0][j] = float(0.5 * (max(lo[j], -3.0) + min(hi[j], 3.0)))
            d.jpos_upper_tols[0][j] = 0.8
            d.jpos_lower_tols[0][j] = -0.8
        return wl
    if name == "max_horizon_64":
        # THIP_MAX_STEPS waypoints, 63 CartPose costs: past the register segment's N <= 32
        # (the generic ADMM step runs)
        return problems.make_workload("B", 4, n_steps=64)
    if name == "min_horizon_2":
        return problems.make_workload("A", 8, n_steps=2)
    if name == "collision_empty_scene":
        wl = problems.make_workload("C", 4)
        wl.desc.n_prims = 0
        wl.scene = np.zeros((wl.batch, 0, 16))
        return wl
    if name == "collision_fixed_both_ends":
        # fixed collision steps at both ends: removeInvalidContactResults drops
        # the contacts at a fixed end (collision_utils.cpp:73-114)
        wl = problems.make_workload("C", 8)
        wl.desc.coll_n_fixed = 2
        wl.desc.coll_fixed_steps[1] = wl.n_steps - 1
        return wl
    if name == "collision_step_subrange":
        wl = problems.make_workload("C", 8)
        wl.desc.coll_first_step = 5
        wl.desc.coll_last_step = 20
        wl.desc.coll_n_fixed = 0
        return wl
    if name == "discrete_fixed_both_ends_subrange":
        # DISCRETE with the last waypoint free (its rows share step pair N - 2) and
        # fixed waypoints inside a sub-range
        wl = _single(problems.make_workload("C", 8, first_problem=40))
        wl.desc.coll_first_step = 3
        wl.desc.coll_last_step = -1
        wl.desc.coll_n_fixed = 2
        wl.desc.coll_fixed_steps[0] = 3
        wl.desc.coll_fixed_steps[1] = 4
        return wl
    if name == "discrete_two_waypoints":
        wl = _single(problems.make_workload("C", 8, n_steps=2, first_problem=60))
        wl.desc.coll_n_fixed = 0
        return wl
    if name == "discrete_with_static_hinges_8dof":
        wl = _single(_variant("collision_with_static_hinges"))
        return wl
    # SQP parity with tolerance bands: free rotation about the tool axis (rx, +-0.2 rad).
    # With bands on all six components the reference algorithm itself is not
    # reproducible (flat cost regions: 1e-13 input perturbations move the oracle's
    # solutions by up to 5e-2 and its costs by 9 %); those bands are covered by the
    # linearisation tests above.
    if name == "cartpose_tolerance_cost":
        return problems.with_cart_tolerances(problems.make_workload("B", 16, first_problem=20), rot=0.2, axes=(3,))
    if name == "cartpose_tolerance_cnt":
        return problems.with_cart_tolerances(problems.make_workload("A", 16, first_problem=20), rot=0.2, axes=(3,))
    if name == "cartpose_tolerance_collision":
        return problems.with_cart_tolerances(problems.make_workload("C", 8, first_problem=20), rot=0.2, axes=(3,))
    if name == "continuous_50_waypoints":
        # config E's horizon and evaluator (50 waypoints, LVS_CONTINUOUS) on the 7-DoF arm: past the
        # register segment's N <= 32, the generic ADMM step with hinge rows
        wl = problems.make_workload("C", 8, n_steps=50, first_problem=30)
        wl.desc.coll_continuous = 1
        return wl
    if name == "jointvel_cnt_band_with_cartpose":
        # config A plus a JointVelIneqConstraint band and a second JointVelIneqCost
        wl = problems.make_workload("A", 16, first_problem=50)
        d = wl.desc
        d.n_jvx = 2
        d.jvx_is_cnt[0], d.jvx_first_step[0], d.jvx_last_step[0] = 1, 0, -1
        d.jvx_is_cnt[1], d.jvx_first_step[1], d.jvx_last_step[1] = 0, 2, 6
        for j in range(wl.n_dof):
            d.jvx_coeffs[0][j], d.jvx_lower_tols[0][j], d.jvx_upper_tols[0][j] = 2.0, -0.15, 0.15
            d.jvx_coeffs[1][j], d.jvx_targets[1][j] = 0.5, 0.02
            d.jvx_lower_tols[1][j], d.jvx_upper_tols[1][j] = -0.01, 0.01
        return wl
    if name == "dynamic_cartpose_costs":
        return problems.with_dynamic_target(problems.make_workload("B", 16, first_problem=70))
    if name == "dynamic_cartpose_cnt_with_collision":
        wl = problems.with_dynamic_target(problems.make_workload("C", 8, first_problem=70))
        wl.desc.cart_is_cnt[5] = 1
        return wl
    if name == "single_problem":
        return problems.make_workload("B", 1, first_problem=5)
    # other chains: 8 DoF with the prismatic torso_lift_joint first, and 6 DoF
    if name == "torso_arm_8dof_A":
        return problems.make_workload("A", 16, robot="torso_right_arm")
    if name == "torso_arm_8dof_B":
        return problems.make_workload("B", 8, robot="torso_right_arm")
    if name == "torso_arm_8dof_C":
        return problems.make_workload("C", 8, robot="torso_right_arm")
    if name == "torso_arm_8dof_jointpos":
        return problems.make_workload("J", 16, robot="torso_right_arm", goal_offset=0.05)
    if name == "arm_6dof_A":
        # square CartPose constraint (6 rows, 6 DoF): several problems stall in the penalty loop and their
        # outcome flips under 1e-13 input perturbations of the oracle itself (problem 9 does)
        return problems.make_workload("A", 16, robot="right_arm_6dof")
    if name == "arm_6dof_C":
        return problems.make_workload("C", 8, robot="right_arm_6dof")
    raise KeyError(name)


VARIANTS = ["jointvel_only", "short_horizon", "two_fixed_steps", "position_only_cartpose", "admm_iteration_cap",
            "sqp_iteration_cap", "sqp_iteration_cap_costs_only", "no_scaling", "no_polish", "no_adaptive_rho_no_warm_start", "single_problem",
            "jointpos_goal", "jointpos_goal_offset", "jointpos_far_goal_penalty_limit", "jointpos_with_cartpose",
            "jointvel_ineq_cost", "jointpos_ineq_cost_and_cnt", "collision_with_static_hinges", "max_horizon_64",
            "min_horizon_2", "collision_empty_scene", "collision_fixed_both_ends", "collision_step_subrange",
            "torso_arm_8dof_A", "torso_arm_8dof_B", "torso_arm_8dof_C", "torso_arm_8dof_jointpos", "arm_6dof_A",
            "arm_6dof_C", "discrete_fixed_both_ends_subrange", "discrete_two_waypoints",
            "discrete_with_static_hinges_8dof", "cartpose_tolerance_cost", "cartpose_tolerance_cnt",
            "cartpose_tolerance_collision", "continuous_50_waypoints", "jointvel_cnt_band_with_cartpose",
            "dynamic_cartpose_costs", "dynamic_cartpose_cnt_with_collision"]


@pytest.mark.parametrize("name", VARIANTS)
def test_sqp_parity_variants(oracle_mod, name):
    wl = _variant(name)
    x, res, _ = solve_gpu(wl)
    # without polishing every QP returns an ADMM iterate: the paths agree
    # only to the ADMM accuracy, so the trajectory bar does not apply
    min_strict = 0.0 if name in ("no_polish", "admm_iteration_cap") else 0.85
    check_parity(wl, oracle_mod, x, res, min_strict=min_strict, label=name)


def test_sqp_iteration_cap_status():
    """optimizers.cpp:922-934: the iteration limit ends the run with
    OPT_SCO_ITERATION_LIMIT while constraints are violated, OPT_CONVERGED
    when there are none (or they are satisfied)."""
    _, res, _ = solve_gpu(_variant("sqp_iteration_cap"))
    assert [r.status for r in res] == [1] * 8 and all(r.n_sqp_iters == 3 for r in res)
    _, res, _ = solve_gpu(_variant("sqp_iteration_cap_costs_only"))
    assert [r.status for r in res] == [0] * 4 and all(r.n_sqp_iters == 3 for r in res)


def test_max_time_zero_ends_before_the_first_iteration(oracle_mod):
    """BasicTrustRegionSQPParameters::max_time (optimizers.cpp:739-753): with 0 the
    check at the top of the first SQP iteration fires before any evaluation, so
    the constraint violations are still empty and the status is OPT_CONVERGED;
    x is the closest feasible point of the start (optimizers.cpp:725)."""
    wl = problems.make_workload("A", 8)
    wl.desc.sqp.max_time = 0.0
    x, res, _ = solve_gpu(wl)
    xo, ro = oracle_mod.solve(wl, n_threads=8)
    for b in range(wl.batch):
        assert res[b].status == ro[b].status == 0
        assert res[b].n_sqp_iters == ro[b].n_sqp_iters == 0 and res[b].n_qp_solves == 0
        assert res[b].total_cost == ro[b].total_cost == 0.0
    np.testing.assert_allclose(x, xo, rtol=0, atol=1e-15)


def test_max_time_limits_the_run():
    """A time limit shorter than the solves: problems end with OPT_TIME_LIMIT
    (constraints violated) or OPT_CONVERGED (none violated), never after more
    SQP iterations than the unlimited run."""
    wl = problems.make_workload("A", 64)
    _, free, _ = solve_gpu(wl)
    wl.desc.sqp.max_time = 2e-4
    _, res, _ = solve_gpu(wl)
    assert any(r.status == 3 for r in res)
    assert all(r.status in (0, 3) or r.n_sqp_iters == f.n_sqp_iters for r, f in zip(res, free))
    assert all(r.n_sqp_iters <= f.n_sqp_iters for r, f in zip(res, free))
    for r in res:
        if r.status == 3:
            assert r.max_cnt_viol >= wl.desc.sqp.cnt_tolerance


# ------------------------------------------------------------------ full size
def _full_size_properties(wl, s, rerun=True):
    """Bitwise-identical reruns (rerun), joint limits, the fixed timestep, statuses, counters."""
    x1, r1 = s.optimize()
    if rerun:
        x2, r2 = s.optimize()
        np.testing.assert_array_equal(x1, x2)
        assert [r.n_admm_iters for r in r1] == [r.n_admm_iters for r in r2]
        assert [r.n_contact_rows for r in r1] == [r.n_contact_rows for r in r2]
    lo, hi, _ = robots.chain_limits(wl.desc.chain)
    # trust-box bounds are clamped to the joint limits; a QP point is feasible
    # to OSQP's tolerance (eps_abs = 1e-4 when it is an unpolished iterate)
    viol = max(float(np.max(lo - x1)), float(np.max(x1 - hi)), 0.0)
    assert viol <= 1e-4, viol
    np.testing.assert_allclose(x1[:, 0], wl.init[:, 0], rtol=0, atol=1e-6)  # fixed timestep rows
    assert all(r.flags == 0 for r in r1)
    assert all(r.status in (0, 1, 2) for r in r1)
    assert all(r.n_sqp_iters >= 1 and r.n_qp_solves >= r.n_sqp_iters for r in r1)
    if wl.desc.coll_enabled:
        assert sum(r.n_contact_rows for r in r1) > 0
        if wl.desc.coll_continuous != 2:
            assert all(r.n_substates >= 2 * (wl.n_steps - 1) * r.n_sqp_iters for r in r1)
    return x1, r1


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("cfg,rank", [("B", 0), ("C", 0), ("C", 7)])
def test_full_batch_every_problem(oracle_mod, cfg, rank):
    """1024 problems per GPU, every problem against the oracle under the strict
    gate: config B, the bench workload (config C), and rank 7's shard of config D
    (configs[3]: 8192 problems over 8 GPUs, seeds 7168-8191, the per-GPU
    workload of the last rank: its whole 1024-problem shard for the
    properties, every 32nd problem against the oracle -- the suite's time
    budget: config C's rank-0 batch is checked on all 1024)."""
    B = 1024
    wl = sharding.rank_workload(cfg, B, rank)
    s = BatchTrustRegionSQP(wl)
    x, res = _full_size_properties(wl, s)
    s.close()
    if rank == 0:
        check_parity(wl, oracle_mod, x, res, label=f"{cfg}-{B}", min_strict=0.9)
        return
    from parity import subset

    idx = np.arange(0, B, 32)
    check_parity(subset(wl, idx), oracle_mod, x[idx], [res[i] for i in idx], label=f"D-rank{rank}-{B}-sample32",
                 min_strict=0.9)


def test_dynamic_problem_assignment_matches_static(hip):
    """Batches larger than the resident slots run persistent workgroups that take
    problems from a counter (KernelArgs::work); the results are bitwise those of
    the one-workgroup-per-problem mapping, run after run (the counter resets
    itself at the end of each launch)."""
    wl = problems.make_workload("A", 600)
    s = BatchTrustRegionSQP(wl)
    x1, r1 = s.optimize()
    x2, r2 = s.optimize()  # a second launch on the same counter
    s.close()
    assert hip.thip_debug_set_path(abi.DEBUG_STATIC_DISPATCH) == 0
    try:
        s = BatchTrustRegionSQP(wl)
        x0, r0 = s.optimize()
        s.close()
    finally:
        hip.thip_debug_set_path(0)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(x2, x0)
    for a, b, c in zip(r0, r1, r2):
        assert (a.status, a.n_sqp_iters, a.n_admm_iters, a.total_cost) == (b.status, b.n_sqp_iters, b.n_admm_iters,
                                                                             b.total_cost)
        assert (b.n_admm_iters, b.total_cost) == (c.n_admm_iters, c.total_cost)


@pytest.mark.timeout(1500)
def test_full_batch_E(oracle_mod):
    """Config E at one GPU's share of configs[4] (4096 problems over 8 GPUs):
    512 problems of the 14-DoF dual arm, 50 waypoints, LVS_CONTINUOUS.
    Properties on every problem (the bitwise rerun is left to the C and B full
    batches: a second 512-problem E launch is ~30 s of the suite's budget), the
    strict gate on 8 problems spread over the batch (the oracle's E solves set
    the suite's time budget)."""
    wl = problems.make_workload("E", 512)
    s = BatchTrustRegionSQP(wl)
    x, res = _full_size_properties(wl, s, rerun=False)
    s.close()
    from parity import subset

    idx = np.arange(0, 512, 64)
    sub = subset(wl, idx)
    check_parity(sub, oracle_mod, x[idx], [res[i] for i in idx], label="E-512-sample8", min_strict=0.85)


def test_devices_stream_interop():
    """The solver runs on a caller-provided torch stream (plumbing for
    overlapping copies with the solve)."""
    import torch

    wl = problems.make_workload("A", 4)
    st = torch.cuda.Stream()
    s = BatchTrustRegionSQP(wl, stream=st.cuda_stream)
    x, res = s.optimize()
    s.close()
    assert all(r.status in (0, 1, 2) for r in res)


# ------------------------------------------------------------------ entry points
def test_smoke_entry():
    import __graft_entry__

    __graft_entry__.smoke()


def test_bench_json_line():
    repo = abi.PKG_DIR.parent
    p = subprocess.run([sys.executable, str(repo / "bench.py"), "--batch", "64", "--steps", "3", "--warmup", "0",
                        "--full", "--cpu-problems", "8"], capture_output=True, text=True, timeout=600, cwd=repo)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] > 0 and line["n_gpus"] == 1 and line["dtype"] == "f64"
    assert line["config"]["batches_in_flight"] == 3 and line["config"]["batch_latency_ms"] > 0
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["limiter"] == "latency" and rf["peak"] == 8000.0 and 0 < rf["frac"] == pytest.approx(rf["achieved"] / 8000.0)
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    assert cb["host_nproc"] >= 1 and cb["single_problem_latency_s"] > 0


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run measures the headline only (the --full fields are null) and
    --dump-outputs writes the last timed step's (x, results) as float64 arrays.
    The inputs are seeded and every problem is solved by one workgroup in a
    fixed order, so the dump equals an in-process solve of the same batch bit
    for bit."""
    repo = abi.PKG_DIR.parent
    p = subprocess.run([sys.executable, str(repo / "bench.py"), "--gpus", "1", "--batch", "64", "--steps", "2",
                        "--warmup", "0", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600, cwd=repo)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "SQP iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["cpu_baseline"] is None and line["config"]["batch_latency_ms"] is None
    assert line["roofline"]["frac"] > 0
    wl = sharding.rank_workload("C", 64, 0)
    x, res, _ = solve_gpu(wl)
    files = {f.stem: np.load(f) for f in (tmp_path / "out").glob("*.npy")}
    assert set(files) == {"x", "problem_index"} | {f"res_{f[0]}" for f in abi.Result._fields_}
    assert all(a.dtype == np.float64 and a.shape[0] == 64 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert np.array_equal(files["problem_index"], np.arange(64))
    print("max |x_dump - x|", np.abs(files["x"] - x).max())
    assert np.array_equal(files["x"], x)
    for f in ("status", "n_sqp_iters", "n_admm_iters", "total_cost"):
        assert np.array_equal(files[f"res_{f}"], np.array([getattr(r, f) for r in res], dtype=np.float64)), f
    assert line["config"]["sqp_iters_per_step"] == int(files["res_n_sqp_iters"].sum())


def test_joint_pos_reference_unit(oracle_mod):
    """joint_costs_unit.cpp:63-150 (equality_jointPos) on the HIP path: the
    reference's EXPECTs plus parity with the oracle."""
    wl = problems.make_reference_unit("joint_pos_eq", 4)
    x, res, _ = solve_gpu(wl)
    for b in range(wl.batch):
        assert res[b].status == 0
        assert np.abs(x[b, 0]).max() < 1e-4
        assert np.abs(x[b, 1:] + 0.1).max() < 0.01
    check_parity(wl, oracle_mod, x, res, label="joint_pos_eq")


def test_joint_pos_ineq_reference_unit(oracle_mod):
    """joint_costs_unit.cpp:152-262 (inequality_jointPos): hinge rows of
    JointPosIneqConstraint / JointPosIneqCost on the HIP path."""
    wl = problems.make_reference_unit("joint_pos_ineq", 4)
    x, res, _ = solve_gpu(wl)
    for b in range(wl.batch):
        assert res[b].status == 0
        for i in list(range(0, 5)) + list(range(6, 10)):
            assert (x[b, i] < 0.2 + 1e-4).all() and (x[b, i] > -0.1 - 1e-4).all()
    check_parity(wl, oracle_mod, x, res, label="joint_pos_ineq")


def test_joint_vel_ineq_reference_unit(oracle_mod):
    """joint_costs_unit.cpp:354-463 (inequality_jointVel): a JointVelIneqConstraint
    and two JointVelIneqCost terms (three JointVel terms, static hinge rows)."""
    wl = problems.make_reference_unit("joint_vel_ineq", 4)
    x, res, _ = solve_gpu(wl)
    N = wl.n_steps
    for b in range(wl.batch):
        assert res[b].n_cnts == 1 and res[b].n_costs == 2
        v = np.diff(x[b], axis=0)
        for i in list(range(0, N // 2)) + list(range(N // 2 + 1, N - 1)):
            assert (v[i] < 0.2 + 1e-4).all() and (v[i] > -0.1 - 1e-4).all()
    check_parity(wl, oracle_mod, x, res, label="joint_vel_ineq")


def test_joint_pos_per_problem_targets():
    """thip_upload_joint_targets: problems with different goals in one batch
    reach their own goals (and the shared-target default is overridden)."""
    wl = problems.make_workload("J", 8)
    assert not np.allclose(wl.jpos_targets[0, 1], wl.jpos_targets[1, 1])
    x, res, _ = solve_gpu(wl)
    for b in range(wl.batch):
        assert res[b].status == 0
        assert np.abs(x[b, -1] - wl.jpos_targets[b, 1]).max() < 1e-4


# ------------------------------------------------------------------ C++ front door
def _lowered_workload(texts, scenes=None):
    """Workload built from the C++ front door's lowering of JSON problems (the
    oracle then solves exactly what the HIP path was given)."""
    from trajopt_amd import host

    parts = [host.lower_json(t, None if scenes is None else scenes[b]) for b, t in enumerate(texts)]
    desc = parts[0][0]
    init = np.stack([p[1] for p in parts])
    tgt = np.stack([p[2] for p in parts])
    jpt = np.stack([p[3] for p in parts]) if desc.n_jpos else None
    sc = np.zeros((len(texts), 0, 16)) if scenes is None else np.asarray(scenes)
    return problems.Workload("json", desc, init, tgt, sc, init.copy(), jpt)


@pytest.mark.parametrize("cfg,B", [("J", 16), ("A", 8), ("C", 4)])
def test_frontdoor_json_batch_parity(oracle_mod, cfg, B):
    """JSON problems -> C++ ProblemConstructionInfo/ConstructProblem ->
    BatchTrustRegionSQP (C++) -> HIP kernel, against the oracle on the same
    lowered problems."""
    from trajopt_amd import host

    wl0 = problems.make_workload(cfg, B)
    texts = [host.workload_to_json(wl0, b) for b in range(B)]
    # JSON problems carry the reference's 0.5 m safety buffer: keep 3 of the
    # 10 primitives so the oracle's QPs stay small enough for a test
    scenes = np.ascontiguousarray(wl0.scene[:, :3]) if wl0.scene.size else None
    x, res = host.solve_json_batch(texts, scenes)
    wl = _lowered_workload(texts, scenes)
    check_parity(wl, oracle_mod, x, res, label=f"json-{cfg}")


def test_frontdoor_reference_planning_config(oracle_mod):
    """The reference's arm_around_table.json (tests/golden/json), unchanged
    (LVS_CONTINUOUS collision cost, JointPos goal constraint), with the table as
    its exact box (Table.stl is a box, tests/dropin_cases.py): parity with the
    oracle, and planning_unit.cpp's EXPECTs -- the initial trajectory in
    collision (:101), OPT_CONVERGED (:125), the final trajectory collision-free
    (:148).  Contact values are not pinned against Bullet (the arm is spheres)."""
    import dropin_cases as dc
    from trajopt_amd import host

    text = dc.text("arm_around_table.json")
    scenes = np.stack([dc.arm_around_table_scene()] * 4)
    x, res = host.solve_json_batch([text] * 4, scenes)
    assert len({r.status for r in res}) == 1
    np.testing.assert_array_equal(x[0], x[3])  # identical problems, identical answers
    wl = _lowered_workload([text] * 4, scenes)
    check_parity(wl, oracle_mod, x, res, label="arm_around_table")
    assert dc.continuous_check_found(wl.desc, wl.init[0], scenes[0], oracle_mod)  # EXPECT_TRUE(found)
    assert res[0].status == 0  # EXPECT_TRUE(status == OPT_CONVERGED)
    assert not dc.continuous_check_found(wl.desc, x[0], scenes[0], oracle_mod)  # EXPECT_FALSE(found)


def test_frontdoor_multi_device_shards():
    """trajopt::MultiDeviceBatchSQP (thost_solve_json_batch_multi): a batch in
    contiguous shards on several device entries -- here three contexts on the
    box's one GPU, each on its own stream, all submitted before any is
    collected -- returns bit for bit the single-context batch, in order, with
    shard sizes differing by at most one (an entry beyond the batch size gets
    nothing)."""
    from trajopt_amd import host

    wl = problems.make_workload("B", 37)
    texts = [host.workload_to_json(wl, b) for b in range(37)]
    x1, r1 = host.solve_json_batch(texts)
    x3, r3 = host.solve_json_batch(texts, devices=[0, 0, 0])
    np.testing.assert_array_equal(x1, x3)
    assert [(a.status, a.n_sqp_iters, a.n_qp_solves, a.total_cost) for a in r1] == \
        [(a.status, a.n_sqp_iters, a.n_qp_solves, a.total_cost) for a in r3]
    x2, _ = host.solve_json_batch(texts[:2], devices=[0, 0, 0])  # one entry idle
    np.testing.assert_array_equal(x2, x1[:2])


def test_frontdoor_stream_batches_in_flight():
    """trajopt::MultiDeviceBatchSQP::optimizeStream (thost_solve_json_stream): 5
    batches with 3 in flight on 2 device entries of the box's GPU (6 contexts,
    each reused for a later batch after its previous one is collected) return
    each batch bit for bit as solved alone, in order."""
    from trajopt_amd import host

    wl = problems.make_workload("B", 5 * 24)
    texts = [host.workload_to_json(wl, b) for b in range(wl.batch)]
    batches = [texts[24 * j:24 * (j + 1)] for j in range(5)]
    xs, rs = host.solve_json_stream(batches, devices=[0, 0], inflight=3)
    for j in range(5):
        x1, r1 = host.solve_json_batch(batches[j])
        np.testing.assert_array_equal(xs[j], x1)
        assert [(a.status, a.n_sqp_iters, a.total_cost) for a in rs[j]] == \
            [(a.status, a.n_sqp_iters, a.total_cost) for a in r1]


def test_frontdoor_cli(tmp_path):
    from trajopt_amd import host

    wl = problems.make_workload("J", 2)
    files = []
    for b in range(2):
        f = tmp_path / f"p{b}.json"
        f.write_text(host.workload_to_json(wl, b))
        files.append(str(f))
    exe = abi.LIB_DIR / "trajopt_batch"
    p = subprocess.run([str(exe), "--repeat", "3", *files], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.count("OPT_CONVERGED") == 6


def test_frontdoor_single_problem_dropin(tmp_path, oracle_mod):
    """trajopt::BasicTrustRegionSQP (the reference's per-problem optimizer usage,
    planning_unit.cpp:83-124: ConstructProblem, initialize, optimize, x()) as a batch of
    one: same trajectory as the oracle on the lowered problem."""
    from trajopt_amd import host

    wl = problems.make_workload("A", 2)
    exe = abi.LIB_DIR / "sqp_single"
    for b in range(2):
        f = tmp_path / f"p{b}.json"
        f.write_text(host.workload_to_json(wl, b))
        p = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        status = lines[0].split()[1]
        x = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
        lw = _lowered_workload([f.read_text()])
        xo, ro = oracle_mod.solve(lw, n_threads=1)
        assert status == ["OPT_CONVERGED", "OPT_SCO_ITERATION_LIMIT", "OPT_PENALTY_ITERATION_LIMIT"][ro[0].status]
        assert np.abs(x - xo[0]).max() <= TOL_X
    # log_results observes the iterations, so the problem takes the host loop (device-evaluated
    # CartPose terms, GpuModel QPs), which writes the reference's four CSV logs: the solver log
    # (writeSolver, optimizers.cpp:533-547) has one line per merit evaluation after the initial
    # one (n_func_evals counts that one too, optimizers.cpp:765-766)
    p = subprocess.run([str(exe), "--log", str(tmp_path), str(f)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    fevals = int(p.stdout.split()[7])
    log = (tmp_path / "trajopt_solver.log").read_text().splitlines()
    assert log[0] == "DESCRIPTION,oldexact,new_exact,dapprox,dexact,ratio"
    assert len(log) == 1 + (fevals - 1) and all(ln.startswith("Solver,") and len(ln.split(",")) == 6 for ln in log[1:])
    for name in ("trajopt_vars.log", "trajopt_costs.log", "trajopt_constraints.log"):
        assert len((tmp_path / name).read_text().splitlines()) >= fevals - 1


def test_contact_capacity_overflow_fails_loudly():
    """A QP with more contacts than coll_max_contacts ends the run with
    OPT_FAILED and THIP_FLAG_CONTACT_OVERFLOW; contacts are never dropped."""
    wl = problems.make_workload("C", 8)
    wl.desc.coll_max_contacts = 4
    _, res, _ = solve_gpu(wl)
    over = [r for r in res if r.flags & 1]
    assert over, "expected at least one problem over 4 contacts"
    assert all(r.status == 4 for r in over)


@pytest.mark.parametrize("cfg,B,path", [("B", 32, abi.DEBUG_NO_SEGMENT), ("C", 32, abi.DEBUG_NO_SEGMENT),
                                         ("B", 32, abi.DEBUG_FORCE_WIDE), ("C", 32, abi.DEBUG_FORCE_WIDE)])
def test_sqp_parity_forced_paths(oracle_mod, cfg, B, path, hip):
    """The generic ADMM step (admm_step + reduced_solve: loads-first loops, masked
    products, per-row-kind updates) and the wide-block solve (block_chain_wide,
    twisted_middle_wide, chain matrices in HBM: config E's path) on problems the
    register-resident segment would otherwise run (thip_debug_set_path): the
    same parity gate against the oracle, and the same outcomes as the segment."""
    wl = problems.make_workload(cfg, B)
    x_seg, res_seg, _ = solve_gpu(wl)
    assert hip.thip_debug_set_path(path) == 0
    try:
        x, res, _ = solve_gpu(wl)
    finally:
        hip.thip_debug_set_path(0)
    name = {abi.DEBUG_NO_SEGMENT: "generic", abi.DEBUG_FORCE_WIDE: "wide"}[path]
    check_parity(wl, oracle_mod, x, res, label=f"{cfg}-{name}")
    same = sum(int(a.status == b.status and np.abs(xa - xb).max() <= TOL_X)
               for a, b, xa, xb in zip(res, res_seg, x, x_seg))
    assert same >= 0.85 * B, f"{cfg}: {name} path and segment agree on {same} of {B} problems"


def test_sqp_parity_dual_arm_E_branches(oracle_mod, hip):
    """The two-branch block solve (Layout::nbr = 2: two independent 7-dof block
    chains) on config E's scene-only variant: without the inter-arm self pairs
    no term couples the arms, so the default layout splits them; against the
    oracle, and against the single 14-dof wide-block solve of the same problems
    (THIP_DEBUG_NO_BRANCH: block_chain_wide, twisted_middle_wide, chain
    matrices in HBM -- the layout config E with its self pairs takes)."""
    from trajopt_amd.runtime import BatchTrustRegionSQP

    wl = problems.make_workload("E", 8)
    wl.desc.n_self_pairs = 0
    s = BatchTrustRegionSQP(wl)
    assert s.layout()["nbr"] == 2 and s.layout()["block_dofs"] == 7, s.layout()
    s.close()
    x_br, res_br, _ = solve_gpu(wl)
    assert hip.thip_debug_set_path(abi.DEBUG_NO_BRANCH) == 0
    try:
        s = BatchTrustRegionSQP(wl)
        assert s.layout()["nbr"] == 1 and s.layout()["wide"] == 1, s.layout()
        s.close()
        x, res, _ = solve_gpu(wl)
    finally:
        hip.thip_debug_set_path(0)
    xo, ro = oracle_mod.solve(wl, n_threads=16)
    for xs, rs, name in ((x_br, res_br, "E-scene-branches"), (x, res, "E-scene-unsplit")):
        assert all(r.flags == 0 for r in rs)
        check_parity(wl, oracle_mod, xs, rs, label=name, oracle=(xo, ro))
    same = sum(int(a.status == b.status and np.abs(xa - xb).max() <= TOL_X) for a, b, xa, xb in zip(res, res_br, x, x_br))
    assert same >= 7, f"unsplit and two-branch solves agree on {same} of 8 problems"


# ------------------------------------------------------------ JointAccEqCost in the fused kernel
# (trajectory_costs.cpp:502-546, JointAccTermInfo::hatch problem_description.cpp:1412-1533):
# P couples waypoints t and t + 2, so the reduced KKT matrix is block-tridiagonal
# over waypoint PAIRS (Layout::grp = 2, 2 D-wide blocks on the wide block path)
def test_joint_acc_runs_the_pair_layout():
    wl = problems.with_joint_acc(problems.make_workload("B", 2))
    s = BatchTrustRegionSQP(wl)
    lay = s.layout()
    s.close()
    assert lay["grp"] == 2 and lay["block_dofs"] == 14 and lay["wide"] == 1 and lay["blocks"] == 15, lay
    assert lay["seg_ok"] == 0 and lay["nbr"] == 1, lay
    # QPs outside the segment's domain run the generic-step build (round 6)
    assert lay["gen"] == 1 and lay["threads"] == 256, lay


@pytest.mark.parametrize("cfg,B", [("HA", 16), ("E", 4), ("C50", 8)])
def test_generic_step_build_matches_main_build(cfg, B):
    """The generic-step build (sqp_kernel_gen: its own compilation without the
    register-resident segment, adaptive unroll in its row / column loops) runs
    the QPs the segment does not take; its results are bitwise those of the
    main build's generic step (THIP_DEBUG_MAIN_BUILD), so the parity checks of
    either cover both."""
    def solve(flags):
        wl = problems.make_workload("C", B, n_steps=50) if cfg == "C50" else problems.make_workload(cfg, B)
        hip = abi.load_hip()
        assert hip.thip_debug_set_path(flags) == 0
        try:
            s = BatchTrustRegionSQP(wl)
            lay = s.layout()
            x, res = s.optimize()
            s.close()
        finally:
            hip.thip_debug_set_path(0)
        return lay, x, [(r.status, r.n_sqp_iters, r.n_admm_iters) for r in res]

    lg, xg, rg = solve(0)
    lm, xm, rm = solve(abi.DEBUG_MAIN_BUILD)
    assert lg["gen"] == 1 and lm["gen"] == 0, (lg, lm)
    assert rg == rm and np.array_equal(xg, xm)


def test_joint_acc_odd_horizon_is_refused():
    """An odd number of waypoints does not pair: thip_create names the generic path."""
    wl = problems.with_joint_acc(problems.make_workload("B", 2, n_steps=29))
    with pytest.raises(HipError) as ei:
        BatchTrustRegionSQP(wl)
    assert "generic path" in str(ei.value)


def _joint_acc_variant(name):
    if name == "B-acc":
        return problems.with_joint_acc(problems.make_workload("B", 32, first_problem=100))
    if name == "C-acc":
        return problems.with_joint_acc(problems.make_workload("C", 16, first_problem=100))
    if name == "A-acc":
        # 10 waypoints, the CartPose constraint on the last one, acceleration cost on steps 2..7
        return problems.with_joint_acc(problems.make_workload("A", 32, first_problem=100), coeff=2.0, target=0.01,
                                       first_step=2, last_step=7)
    if name == "J-acc-8dof":
        return problems.with_joint_acc(problems.make_workload("J", 16, robot="torso_right_arm", goal_offset=0.05),
                                       coeff=0.5)
    if name == "B-acc-two-terms":
        wl = problems.with_joint_acc(problems.make_workload("B", 16, first_problem=140), coeff=1.0)
        return problems.with_joint_acc(wl, coeff=3.0, target=-0.002, first_step=10, last_step=20)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["B-acc", "C-acc", "A-acc", "J-acc-8dof", "B-acc-two-terms"])
def test_sqp_parity_joint_acc(oracle_mod, name):
    wl = _joint_acc_variant(name)
    x, res, _ = solve_gpu(wl)
    assert all(r.flags == 0 for r in res)
    check_parity(wl, oracle_mod, x, res, label=name)


def test_joint_acc_reference_unit_cost(oracle_mod):
    """joint_costs_unit.cpp:677-766 (equality_jointAcc), its cost part: JointAcc
    coefficient 10 targeting 0.1 on every step of a 10-waypoint stationary start
    (the PR2 right arm at rest); EXPECT_NEAR(accel, 0.1, 0.01) on every step, and
    parity with the oracle (the unit's zero-acceleration constraint on step 0 is an
    abs row over three waypoints: the generic path runs that form)."""
    wl = problems.make_workload("J", 4)
    d = wl.desc
    d.n_jpos = 0
    d.n_fixed = 0
    d.jv_enabled = 0
    for j in range(wl.n_dof):  # a stationary start in the middle of each joint's range
        lo, hi = d.chain.lower[j], d.chain.upper[j]
        wl.init[:, :, j] = 0.5 * (lo + hi) if hi - lo < 10 else 0.0
    problems.with_joint_acc(wl, coeff=10.0, target=0.1)
    x, res, _ = solve_gpu(wl)
    for b in range(wl.batch):
        acc = x[b, :-2] - 2 * x[b, 1:-1] + x[b, 2:]
        assert np.abs(acc - 0.1).max() < 0.01, np.abs(acc - 0.1).max()
    check_parity(wl, oracle_mod, x, res, label="jointacc-unit-cost", min_strict=0.0)


def test_zz_pooled_strict_fraction():
    """Pooled over every parity check of the session that carries a fraction
    bound: at least 93 % of all problems meet the bar strictly (the rest carry
    a per-problem proof of oracle instability)."""
    strict, total = pooled()
    if total < 200:
        pytest.skip(f"only {total} problems checked in this session")
    assert strict >= 0.93 * total, f"pooled strict fraction {strict}/{total}"
